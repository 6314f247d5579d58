// step_fuse.h — host-side bookkeeping of a multi-step launch (plain C++, no HIP).
//
// A multi-step launch of step_kernel runs up to kFuseMax consecutive control
// steps of the same envs; step j writes through its own set of output
// pointers.  Waves of one launch are at different steps at the same moment, so
// no output range of a step may overlap an output range of another step of the
// same launch (within one step the caller's buffers are what they are for a
// single step).  FuseGroup collects the steps of one launch under that rule;
// qs_step uses it to grow a kernel node of a stream capture (capture id,
// stream and node say which), qs_step_many to cut its steps into launches.
#pragma once

#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kFuseMax = 32;    // = kMaxFuse (step_kernel.h), checked in quadswarm.hip
constexpr int kFuseOuts = 7;    // obs, reward, terminated, truncated, terminal_obs, reasons, actions_out

struct FuseOuts {
  const void* p[kFuseOuts];
};

// May a multi-step launch take the kernel's fast obs path (ParamsMany::obs_pipe)?
// There a workgroup's obs rows of a step wait in LDS and leave as whole float4
// pieces of one contiguous span during the next step, so:
//  - the kernel instance is one with the compile-time control frequency
//    (`fixed_cf`; the others do not carry the path),
//  - a row is at most kObsPipeMaxRow floats (a lane holds ⌈row/4⌉ float4 in flight),
//  - a workgroup holds kObsPipeRows `rows` (= envs per workgroup × drones: every
//    lane of the wave a drone), so the pieces' offsets are constants and the
//    span, rows × row_floats floats, is a whole number of float4 that starts a
//    multiple of 16 bytes from the buffer's start in every workgroup,
//  - all of them are staged in one pass,
//  - every obs buffer of the launch is 16-byte aligned (a step may have none).
// Any other launch takes the general path.
constexpr int kObsPipeMaxRow = 32;   // = kObsPipeMaxO (step_kernel.h), checked in quadswarm.hip
constexpr int kObsPipeRows = 64;     // = kBlock (step_kernel.h), checked in quadswarm.hip
inline bool obs_pipe_ok(bool fixed_cf, int stage_rows, int rows, int row_floats, const void* const* obs, int nsteps) {
  if (!fixed_cf || rows != kObsPipeRows || row_floats <= 0 || row_floats > kObsPipeMaxRow) return false;
  if (stage_rows < rows) return false;
  for (int j = 0; j < nsteps; ++j)
    if (obs[j] && ((uintptr_t)obs[j] & 15u) != 0) return false;
  return true;
}

// May a multi-step launch of the synthetic policy run the shape-specialised
// kernel instance (step_kernel HOT = 1, step_mh_hot.hip)?  That instance has
// folded in, as constants, everything listed here; a launch that differs in any
// of it takes the general instance:
//  - MultiHover, ONE_D_PID, the compile-time control frequency (`fixed_cf`:
//    30 Hz at 240, not DroneModel.CF2P), DYN or PYB physics, no extra forces,
//    auto-reset on (neither QS_FLAG_NO_AUTORESET nor QS_FLAG_CF2P set),
//  - kHotDrones drones, kHotEnvs envs per workgroup and a number of envs that
//    fills every workgroup (no idle lane anywhere in the grid),
//  - a reject-free layout (a reset is try 0) and neither a deferred search queue
//    nor precomputed searches,
//  - the per-env reduction inside the wave (QS_WAVE_REDUCE) and the fast obs path
//    (obs_pipe_ok's verdict for this launch, which covers the obs alignment),
//  - at least two steps, and at every step of the launch the same outputs: obs,
//    reward, terminated, truncated and actions_out present, terminal_obs and
//    reasons absent (kHotOutMask over FuseOuts' order).
// The values of quadswarm.h's enums are restated as plain ints (this header
// stays free of it); quadswarm.hip checks them against the header's.
constexpr int kHotTask = 0, kHotAct = 4;             // QS_TASK_MULTIHOVER, QS_ACT_ONE_D_PID
constexpr int kHotPhysA = 0, kHotPhysB = 1;          // QS_PHYS_PYB, QS_PHYS_DYN
constexpr unsigned kHotBadFlags = 1u | 4u;           // QS_FLAG_NO_AUTORESET | QS_FLAG_CF2P
constexpr int kHotDrones = 8, kHotEnvs = 8;          // = kHotD, kBlock / kHotD (step_kernel.h)
constexpr unsigned kHotOutMask = 1u | 2u | 4u | 8u | 64u;   // obs, reward, terminated, truncated, actions_out

inline unsigned out_mask(const FuseOuts& o) {
  unsigned m = 0;
  for (int i = 0; i < kFuseOuts; ++i)
    if (o.p[i]) m |= 1u << i;
  return m;
}

struct HotShape {
  int task, act_type;
  bool fixed_cf;
  int physics;
  unsigned aux, flags;
  int D, E, EPB;
  bool reject_free, reset_queue, reset_pre, wave_reduce, obs_pipe;
};

inline bool hot_shape_ok(const HotShape& s, const unsigned* out_masks, int nsteps) {
  if (s.task != kHotTask || s.act_type != kHotAct || !s.fixed_cf) return false;
  if (s.physics != kHotPhysA && s.physics != kHotPhysB) return false;
  if (s.aux != 0 || (s.flags & kHotBadFlags) != 0) return false;
  if (s.D != kHotDrones || s.EPB != kHotEnvs || s.E <= 0 || s.E % s.EPB != 0) return false;
  if (!s.reject_free || s.reset_queue || s.reset_pre || !s.wave_reduce || !s.obs_pipe) return false;
  if (nsteps < 2 || nsteps > kFuseMax || !out_masks) return false;
  for (int j = 0; j < nsteps; ++j)
    if (out_masks[j] != kHotOutMask) return false;
  return true;
}

// A launch may go on past its distinct output sets when the further steps write
// those sets again in the same order (a ring of P sets: step k of the launch
// writes set k mod P).  Safe because a workgroup writes only its own envs' rows of
// every output, a wave's stores to one address retire in program order, and
// nothing in a launch reads what it wrote: after the launch every set holds what
// the last step that wrote it produced, as after a chain of single steps.  Only
// the ring instance of the kernel (step_kernel HOT = 2, step_mh_ring.hip) runs
// such a launch, so only the hot shape wraps (ring_shape_ok); kRingMaxSteps caps
// the steps of one launch.
constexpr int kRingMaxSteps = 1024;

// hot_shape_ok over the `period` distinct sets of a launch of `total` steps that
// has wrapped at least once.
inline bool ring_shape_ok(const HotShape& s, const unsigned* out_masks, int period, int total) {
  return hot_shape_ok(s, out_masks, period) && total > period && total <= kRingMaxSteps;
}

struct FuseGroup {
  bool live = false;
  unsigned long long capture_id = 0;   // the stream capture the node belongs to
  void* stream = nullptr;
  void* node = nullptr;                // the kernel node that holds `count` steps
  int count = 0;                       // distinct output sets held (outs[0 .. count-1])
  int period = 0;                      // 0 until a wrap; then the ring's length (= count, which no longer grows)
  int total = 0;                       // steps held: count, plus the wrapped ones
  size_t bytes[kFuseOuts] = {0, 0, 0, 0, 0, 0, 0};   // size of each output a step writes
  FuseOuts outs[kFuseMax];

  void forget() {
    live = false;
    node = nullptr;
    stream = nullptr;
    count = 0;
    period = 0;
    total = 0;
  }

  // A new group whose first step writes `o`.
  void begin(const size_t sizes[kFuseOuts], const FuseOuts& o, unsigned long long id = 0, void* st = nullptr,
             void* nd = nullptr) {
    for (int i = 0; i < kFuseOuts; ++i) bytes[i] = sizes[i];
    outs[0] = o;
    count = 1;
    period = 0;
    total = 1;
    capture_id = id;
    stream = st;
    node = nd;
    live = true;
  }

  static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
  }

  // Every non-null output range of `o` is disjoint from every non-null output
  // range of the steps already in the group.
  bool distinct(const FuseOuts& o) const {
    for (int i = 0; i < kFuseOuts; ++i) {
      if (!o.p[i]) continue;
      for (int s = 0; s < count; ++s)
        for (int j = 0; j < kFuseOuts; ++j)
          if (outs[s].p[j] && overlap(o.p[i], bytes[i], outs[s].p[j], bytes[j])) return false;
    }
    return true;
  }

  // May a further step with outputs `o` join, at fusion depth `depth`?
  bool can_append(const FuseOuts& o, int depth) const {
    const int cap = depth < kFuseMax ? depth : kFuseMax;
    return live && count >= 1 && count < cap && distinct(o);
  }

  // The same for the node of a capture: the caller's stream must still be in
  // the capture that made the node.  (Compared before the node is touched: a
  // node of an ended capture may be gone.)
  bool same_capture(unsigned long long id, const void* st) const {
    return live && node != nullptr && id == capture_id && st == stream;
  }

  void append(const FuseOuts& o) {
    outs[count] = o;
    count += 1;
    total += 1;
  }

  static bool same_set(const FuseOuts& a, const FuseOuts& b) {
    for (int i = 0; i < kFuseOuts; ++i)
      if (a.p[i] != b.p[i]) return false;
    return true;
  }

  // May a further step whose outputs `o` overlap the group's join it as the next
  // step of a ring?  Only if it writes exactly the set that is due: all seven
  // pointers, NULLs included, those of outs[total mod P], where P is the period
  // (before the first wrap the number of sets held, and then the set due is
  // outs[0]).  At least two sets, at most min(depth, kFuseMax) of them, and fewer
  // than `max_total` (and kRingMaxSteps) steps so far.  Anything else cuts the
  // launch: a set out of turn, one pointer that differs, a partial overlap, one
  // buffer set reused every step (P = 1).  Once a group has wrapped it takes no
  // new set: the caller asks can_append only while period == 0.
  bool can_wrap(const FuseOuts& o, int depth, int max_total) const {
    const int cap = depth < kFuseMax ? depth : kFuseMax;
    const int lim = max_total < kRingMaxSteps ? max_total : kRingMaxSteps;
    if (!live || count < 2 || count > cap || total < count || total >= lim) return false;
    if (period == 0 ? total != count : period != count) return false;
    return same_set(o, outs[total % count]);
  }

  void wrap() {
    period = count;
    total += 1;
  }
};

// A multi-step launch whose steps read caller-supplied actions (qs_step_seq).
// The kernel reads the action rows of all its steps before the first step
// runs, and its waves are at different steps at the same moment, so on top of
// FuseGroup's rule a step joins only if
//  - its action range is disjoint from every non-null output range of every
//    step already in the group (else it would read what an earlier step of the
//    launch has yet to write), and
//  - each of its non-null output ranges is disjoint from the action range of
//    every step already in the group (reads, once a launch runs, come first).
// Cutting the launch before such a step restores the order of single steps.
// Steps that read the same or overlapping actions may share a launch (nobody
// writes them), and a step's own actions against its own outputs are what they
// are for a single step.
struct SeqGroup {
  FuseGroup g;
  size_t act_bytes = 0;              // N·A·4: the bytes of an action buffer a step reads
  const void* acts[kFuseMax];

  int count() const { return g.count; }

  void begin(const size_t sizes[kFuseOuts], const FuseOuts& o, const void* act, size_t act_size) {
    g.begin(sizes, o);
    act_bytes = act_size;
    acts[0] = act;
  }

  bool can_append(const FuseOuts& o, const void* act, int depth) const {
    if (!g.can_append(o, depth)) return false;
    for (int s = 0; s < g.count; ++s) {
      for (int j = 0; j < kFuseOuts; ++j)
        if (g.outs[s].p[j] && FuseGroup::overlap(act, act_bytes, g.outs[s].p[j], g.bytes[j])) return false;
      for (int i = 0; i < kFuseOuts; ++i)
        if (o.p[i] && FuseGroup::overlap(o.p[i], g.bytes[i], acts[s], act_bytes)) return false;
    }
    return true;
  }

  void append(const FuseOuts& o, const void* act) {
    acts[g.count] = act;
    g.append(o);
  }
};

// The depth of such a launch.  Its action rows wait in LDS, kSeqStepBytes · A
// bytes per step and one-wave workgroup ([step][component][lane] dwords), beside
// the obs stage.  `share_free`: what a workgroup's share of the CU's LDS has left
// when the launch's workgroups are all to be resident at once; `cu_free`: what is
// left when a workgroup may take the whole CU's.  Residency is worth more than
// depth (a grid that runs in two rounds pays every step twice), but below
// kSeqMinDepth steps a launch has little left to share, so that many are taken
// from `cu_free` where they fit.  Never more than `depth` or kFuseMax, never
// fewer than 1 (= a single step, which reads its actions from HBM).
constexpr int kSeqStepBytes = kObsPipeRows * 4;
constexpr int kSeqMinDepth = 4;
inline int seq_depth_cap(size_t share_free, size_t cu_free, int act_dim, int depth) {
  const size_t per_step = (size_t)kSeqStepBytes * (size_t)(act_dim > 0 ? act_dim : 1);
  size_t k = share_free / per_step;
  if (k < (size_t)kSeqMinDepth) {
    const size_t kc = cu_free / per_step;
    const size_t floor_k = kc < (size_t)kSeqMinDepth ? kc : (size_t)kSeqMinDepth;
    if (floor_k > k) k = floor_k;
  }
  const size_t cap = (size_t)(depth < kFuseMax ? depth : kFuseMax);
  if (k > cap) k = cap;
  return k < 1 ? 1 : (int)k;
}

}  // namespace qs
