// step_branch.h — host-side arithmetic of a branch set (qs_branch_*; plain C++,
// no HIP).
//
// A branch set keeps the state of C · E virtual envs (virtual env v = c · E + e,
// as in qs_score) in device memory of its own, so that a branch rollout can be
// carried from one launch to the next: qs_branch_fork copies the handle's envs
// into it, qs_branch_advance runs up to qs_score_depth steps of the FUSE = 4 step
// kernel on it, qs_branch_select regroups it.  Three things are plain
// arithmetic and live here: how large the set's blocks are and whether the
// kernels' 32-bit offsets reach them, how a rollout of any length is cut into
// launches, and the live / first-done rule of the accumulators, as the
// reference the kernel's bookkeeping is tested against.
#pragma once

#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kBranchEnvRec = 8;       // = kEnvRec (step_kernel.h), checked in quadswarm.hip: int32 words of an env record
constexpr int kBranchBlocks = 6;       // agent, env, history, ret, first_done, ret_agent
constexpr uint64_t kBranchAlign = 256; // every block starts on its own 256-byte line

// A set of C candidates over a handle of E envs × D drones: `fields` agent
// fields of `real_bytes` each, a history ring of H slots × A floats per agent.
struct BranchShape {
  int64_t C, E, D, H, A, fields, real_bytes;
};
// Bytes of the six blocks, in the order agent [fields][N], env records
// [V][kBranchEnvRec] int32, history [H][N][A] float32, ret [V] double, first_done
// [V] int32, ret_agent [N] double; V = C · E virtual envs, N = V · D agents.
struct BranchSizes {
  uint64_t V, N;
  uint64_t bytes[kBranchBlocks];
  uint64_t offset[kBranchBlocks];   // of each block in one allocation (kBranchAlign apart at least)
  uint64_t total;                   // bytes of that allocation
};
// false: a bad shape, or a block the kernels could not address.  The step kernel
// indexes agents with 32-bit integers and reaches each block through a buffer
// descriptor whose byte range is a signed 32-bit value, so V, N and every block's
// bytes must stay below 2^31 (written like score_sizes in step_score.h: no
// product is formed before its factors are known to be small).
inline bool branch_sizes(const BranchShape& s, BranchSizes* out) {
  if (s.C < 1 || s.E < 1 || s.D < 1 || s.H < 1 || s.A < 1 || s.fields < 1 || s.real_bytes < 1) return false;
  const uint64_t lim = uint64_t(1) << 31;
  if ((uint64_t)s.C >= lim || (uint64_t)s.E >= lim || (uint64_t)s.D >= lim) return false;
  const uint64_t V = (uint64_t)s.C * (uint64_t)s.E;   // C, E < 2^31: no overflow
  if (V >= lim) return false;
  const uint64_t N = V * (uint64_t)s.D;               // V, D < 2^31
  if (N >= lim) return false;
  if ((uint64_t)s.fields >= lim || (uint64_t)s.real_bytes >= lim || (uint64_t)s.H >= lim || (uint64_t)s.A >= lim) return false;
  const uint64_t per_agent = (uint64_t)s.fields * (uint64_t)s.real_bytes;   // < 2^62
  const uint64_t per_hist = (uint64_t)s.H * (uint64_t)s.A;                  // < 2^62
  if (per_agent >= lim || per_hist * 4u >= lim) return false;               // then N · either < 2^62
  out->V = V;
  out->N = N;
  out->bytes[0] = N * per_agent;
  out->bytes[1] = V * (uint64_t)kBranchEnvRec * 4u;
  out->bytes[2] = N * per_hist * 4u;
  out->bytes[3] = V * 8u;
  out->bytes[4] = V * 4u;
  out->bytes[5] = N * 8u;
  uint64_t at = 0;
  for (int i = 0; i < kBranchBlocks; ++i) {
    if (out->bytes[i] >= lim) return false;
    out->offset[i] = at;
    at += (out->bytes[i] + kBranchAlign - 1) / kBranchAlign * kBranchAlign;
  }
  out->total = at;
  return true;
}

// A rollout of `remaining` more steps on a handle of depth `depth` (>= 1): the
// steps of its next launch.  Every launch but the last is a full one.
inline int branch_chunk(int64_t remaining, int depth) {
  if (remaining < 1 || depth < 1) return 0;
  return remaining < (int64_t)depth ? (int)remaining : depth;
}
// … and how many launches it takes in all.
inline int64_t branch_launches(int64_t total, int depth) {
  if (total < 1 || depth < 1) return 0;
  return (total + depth - 1) / depth;
}
// first_done is an int32 step index since the fork: an advance of n steps at
// `steps` must leave steps + n representable.
inline bool branch_steps_fit(int64_t steps, int n) {
  return steps >= 0 && n >= 0 && steps + (int64_t)n <= (int64_t)INT32_MAX;
}

// The accumulators of one env of one candidate.  An env is live at step index
// t iff first_done == t: it has not been done since the fork.  An advance of n
// steps from t adds, while the env is live, each step's reward in step order;
// the first done step j freezes them with first_done = t + j, and an env still
// live afterwards has first_done = t + n.  (What the FUSE = 4 kernel does with the
// values it loads and stores; a chain of advances gives what one long advance gives.)
struct BranchAcc {
  double ret = 0;
  int32_t first_done = 0;
};
inline void branch_accumulate(BranchAcc& a, int64_t t, int n, const double* reward, const uint8_t* done) {
  if ((int64_t)a.first_done != t) return;   // frozen before this launch
  for (int j = 0; j < n; ++j) {
    a.ret += reward[j];
    if (done[j]) {
      a.first_done = (int32_t)(t + j);
      return;
    }
  }
  a.first_done = (int32_t)(t + n);
}

}  // namespace qs
