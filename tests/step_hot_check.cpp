// Stand-alone host check of qs::hot_shape_ok (csrc/step_fuse.h; no GPU, no HIP):
// which multi-step launches may run the shape-specialised kernel instance.  Built
// and run by tests/test_step_hot_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "step_fuse.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

namespace {
// the values of include/quadswarm.h that the cases name
constexpr int kTaskMultiHover = 0, kTaskSpiral = 1, kActVel = 2, kActOneDPid = 4, kPhysPyb = 0, kPhysDyn = 1;
constexpr unsigned kFlagNoAutoreset = 1u, kFlagInKernelSearch = 2u, kFlagCf2p = 4u;

// The flagship launch: MultiHover, ONE_D_PID, 30 Hz, DYN, 8 drones × 16 384 envs.
qs::HotShape flagship() {
  return qs::HotShape{kTaskMultiHover, kActOneDPid, true, kPhysDyn, 0u, 0u, 8, 16384, 8, true, false, false, true, true};
}

// A step's outputs as the host sees them (FuseOuts order: obs, reward, terminated,
// truncated, terminal_obs, reasons, actions_out) out of one arena, 16-byte aligned.
struct Arena {
  alignas(64) float mem[qs::kFuseMax * 7 * 64 + 16];
  qs::FuseOuts step(int j) const {
    qs::FuseOuts o{};
    for (int i = 0; i < qs::kFuseOuts; ++i) o.p[i] = mem + (j * 7 + i) * 64;
    o.p[4] = nullptr;   // terminal_obs
    o.p[5] = nullptr;   // reasons
    return o;
  }
};

// The host's two decisions for a launch, as quadswarm.hip makes them: the fast
// obs path from the obs pointers, then the hot shape with that verdict in it.
bool decide(qs::HotShape s, const std::vector<qs::FuseOuts>& outs) {
  const int n = (int)outs.size();
  std::vector<const void*> obs(n);
  std::vector<unsigned> masks(n);
  for (int j = 0; j < n; ++j) {
    obs[j] = outs[j].p[0];
    masks[j] = qs::out_mask(outs[j]);
  }
  s.obs_pipe = qs::obs_pipe_ok(s.fixed_cf, 64, s.EPB * s.D, 27, obs.data(), n);
  return qs::hot_shape_ok(s, masks.data(), n);
}
}  // namespace

int main() {
  static Arena A;
  std::vector<qs::FuseOuts> outs;
  for (int j = 0; j < qs::kFuseMax; ++j) outs.push_back(A.step(j));
  auto first = [&](int n) { return std::vector<qs::FuseOuts>(outs.begin(), outs.begin() + n); };

  // the flagship shape, at every depth of two or more steps; PYB and other env counts that fill the waves
  CHECK(decide(flagship(), outs));
  for (int n = 2; n <= qs::kFuseMax; ++n) CHECK(decide(flagship(), first(n)));
  { qs::HotShape s = flagship(); s.physics = kPhysPyb; CHECK(decide(s, outs)); }
  for (int E : {8, 24, 4096}) { qs::HotShape s = flagship(); s.E = E; CHECK(decide(s, first(4))); }
  CHECK(qs::out_mask(outs[0]) == qs::kHotOutMask);

  // one deviation each
  for (int D : {4, 16}) {   // other drone counts (with their own envs per wave)
    qs::HotShape s = flagship(); s.D = D; s.EPB = 64 / D;
    CHECK(!decide(s, outs));
    s.EPB = 8;
    CHECK(!decide(s, outs));
  }
  for (int E : {12, 1, 7, 16385}) { qs::HotShape s = flagship(); s.E = E; CHECK(!decide(s, outs)); }   // a partial workgroup
  { qs::HotShape s = flagship(); s.EPB = 4; CHECK(!decide(s, outs)); }        // halved envs per wave
  for (int bad : {0, 2, 17, qs::kFuseMax - 1}) {   // one step of 32 without a reward
    std::vector<qs::FuseOuts> m = outs;
    m[bad].p[1] = nullptr;
    CHECK(!decide(flagship(), m));
    if (bad >= 2) CHECK(decide(flagship(), std::vector<qs::FuseOuts>(m.begin(), m.begin() + bad)));   // the steps before it qualify
  }
  for (int out : {0, 2, 3, 6}) {   // … or without obs, terminated, truncated, actions_out
    std::vector<qs::FuseOuts> m = outs;
    m[5].p[out] = nullptr;
    CHECK(!decide(flagship(), m));
  }
  {   // one step with terminal_obs; one with reasons; every step with them
    std::vector<qs::FuseOuts> m = outs;
    m[9].p[4] = A.mem + 8;
    CHECK(!decide(flagship(), m));
    m = outs;
    m[31].p[5] = A.mem + 8;
    CHECK(!decide(flagship(), m));
    m = outs;
    for (auto& o : m) { o.p[4] = A.mem; o.p[5] = A.mem; }
    CHECK(!decide(flagship(), m));
  }
  for (int off = 1; off < 4; ++off) {   // one misaligned obs (4, 8, 12 bytes)
    std::vector<qs::FuseOuts> m = outs;
    m[3].p[0] = (const float*)m[3].p[0] + off;
    CHECK(!decide(flagship(), m));
  }
  { qs::HotShape s = flagship(); s.act_type = kActVel; CHECK(!decide(s, outs)); }
  for (int act : {0, 1, 3}) { qs::HotShape s = flagship(); s.act_type = act; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.task = kTaskSpiral; CHECK(!decide(s, outs)); }
  for (int task : {2, 3, 4}) { qs::HotShape s = flagship(); s.task = task; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.flags = kFlagCf2p; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.flags = kFlagNoAutoreset; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.flags = kFlagInKernelSearch; CHECK(decide(s, outs)); }   // (moot on a reject-free layout)
  { qs::HotShape s = flagship(); s.reset_queue = true; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.reset_pre = true; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.reject_free = false; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.wave_reduce = false; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.fixed_cf = false; CHECK(!decide(s, outs)); }    // a run-time control frequency
  for (unsigned aux : {1u, 2u, 4u, 7u}) { qs::HotShape s = flagship(); s.aux = aux; CHECK(!decide(s, outs)); }
  { qs::HotShape s = flagship(); s.physics = 2; CHECK(!decide(s, outs)); }
  CHECK(!decide(flagship(), first(1)));                                             // nsteps = 1
  {   // the predicate itself: no steps, too many, no masks, the obs verdict withheld
    const std::vector<unsigned> masks(qs::kFuseMax + 1, qs::kHotOutMask);
    CHECK(qs::hot_shape_ok(flagship(), masks.data(), qs::kFuseMax));
    CHECK(!qs::hot_shape_ok(flagship(), masks.data(), 0));
    CHECK(!qs::hot_shape_ok(flagship(), masks.data(), qs::kFuseMax + 1));
    CHECK(!qs::hot_shape_ok(flagship(), nullptr, 4));
    qs::HotShape s = flagship();
    s.obs_pipe = false;
    CHECK(!qs::hot_shape_ok(s, masks.data(), 4));
  }
  std::printf("step_hot ok\n");
  return 0;
}
