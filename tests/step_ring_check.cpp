// Stand-alone host check of qs::FuseGroup::can_wrap and qs::ring_shape_ok
// (csrc/step_fuse.h; no GPU, no HIP): which steps may stay in a launch that has
// run out of distinct output sets because they write those sets again in order.
// Built and run by tests/test_step_ring_host.py with -fsanitize=address,undefined.
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
constexpr int kSets = qs::kFuseMax + 2;
// A step's outputs (FuseOuts order) out of one arena, 64 floats each; terminal_obs
// and reasons absent, as the hot shape has them.
struct Arena {
  alignas(64) float mem[kSets * 7 * 64 + 64];
  qs::FuseOuts set(int j) const {
    qs::FuseOuts o{};
    for (int i = 0; i < qs::kFuseOuts; ++i) o.p[i] = mem + (j * 7 + i) * 64;
    o.p[4] = nullptr;
    o.p[5] = nullptr;
    return o;
  }
};
const size_t kSizes[qs::kFuseOuts] = {256, 256, 256, 256, 256, 256, 256};

// A group that holds sets 0 .. n-1, grown as the library grows it.
bool grow(qs::FuseGroup& g, const Arena& A, int n, int depth) {
  g.begin(kSizes, A.set(0));
  for (int j = 1; j < n; ++j) {
    if (!g.can_append(A.set(j), depth)) return false;
    g.append(A.set(j));
  }
  return g.count == n && g.total == n && g.period == 0;
}

// The flagship launch: MultiHover, ONE_D_PID, 30 Hz, DYN, 8 drones × 16 384 envs.
qs::HotShape flagship() {
  return qs::HotShape{0, 4, true, 1, 0u, 0u, 8, 16384, 8, true, false, false, true, true};
}
}  // namespace

int main() {
  static Arena A;
  const int kMax = qs::kRingMaxSteps;

  // the first wrap and every later position, for several periods: the set due is outs[total mod P]
  for (int P : {2, 3, 7, qs::kFuseMax}) {
    qs::FuseGroup g;
    CHECK(grow(g, A, P, qs::kFuseMax));
    CHECK(!g.can_append(A.set(0), qs::kFuseMax));   // (it overlaps: the launch would be cut here)
    for (int t = P; t < 5 * P + 1; ++t) {
      for (int j = 0; j < P; ++j) CHECK(g.can_wrap(A.set(j), qs::kFuseMax, kMax) == (j == t % P));
      CHECK(!g.can_wrap(A.set(P), qs::kFuseMax, kMax));   // a set the group does not hold
      g.wrap();
      CHECK(g.period == P && g.count == P && g.total == t + 1);
    }
  }

  // refusals
  {
    qs::FuseGroup g;   // not live
    CHECK(!g.can_wrap(A.set(0), qs::kFuseMax, kMax));
    CHECK(grow(g, A, 1, qs::kFuseMax));   // one buffer set reused every step (P = 1)
    CHECK(!g.can_wrap(A.set(0), qs::kFuseMax, kMax));
    g.forget();
    CHECK(!g.can_wrap(A.set(0), qs::kFuseMax, kMax) && g.period == 0 && g.total == 0);
  }
  {
    qs::FuseGroup g;
    CHECK(grow(g, A, 3, qs::kFuseMax));
    CHECK(!g.can_wrap(A.set(1), qs::kFuseMax, kMax));   // outs[1] where outs[0] was due
    CHECK(!g.can_wrap(A.set(2), qs::kFuseMax, kMax));
    for (int i = 0; i < qs::kFuseOuts; ++i) {            // one pointer that differs (a NULL for a buffer, a buffer for a NULL)
      qs::FuseOuts o = A.set(0);
      o.p[i] = o.p[i] ? nullptr : (const void*)(A.mem + kSets * 7 * 64);
      CHECK(!g.can_wrap(o, qs::kFuseMax, kMax));
      o = A.set(0);
      o.p[i] = A.set(5).p[1];                            // … or another buffer (same obs, another reward)
      CHECK(!g.can_wrap(o, qs::kFuseMax, kMax));
    }
    {                                                    // a partial overlap
      qs::FuseOuts o = A.set(0);
      o.p[0] = (const float*)o.p[0] + 4;
      CHECK(!g.can_wrap(o, qs::kFuseMax, kMax));
    }
    CHECK(g.can_wrap(A.set(0), qs::kFuseMax, kMax));
    g.wrap();
    CHECK(!g.can_wrap(A.set(0), qs::kFuseMax, kMax));   // after the wrap: set 1 is due
    CHECK(!g.can_wrap(A.set(2), qs::kFuseMax, kMax));
    CHECK(g.can_wrap(A.set(1), qs::kFuseMax, kMax));
  }

  // the cap: max_total, and kRingMaxSteps whatever max_total says
  {
    qs::FuseGroup g;
    CHECK(grow(g, A, 3, qs::kFuseMax));
    int t = 3;
    while (g.can_wrap(A.set(t % 3), qs::kFuseMax, 10)) { g.wrap(); ++t; }
    CHECK(t == 10 && g.total == 10);
    CHECK(g.can_wrap(A.set(10 % 3), qs::kFuseMax, 11));
    CHECK(!g.can_wrap(A.set(0), qs::kFuseMax, 3) && !g.can_wrap(A.set(0), qs::kFuseMax, 0));
    while (g.can_wrap(A.set(t % 3), qs::kFuseMax, 1 << 20)) { g.wrap(); ++t; }
    CHECK(t == qs::kRingMaxSteps && g.total == qs::kRingMaxSteps);
    qs::FuseGroup f;   // a group already at the cap when its sets run out
    CHECK(grow(f, A, 3, qs::kFuseMax));
    CHECK(!f.can_wrap(A.set(0), qs::kFuseMax, 3));
    CHECK(f.can_wrap(A.set(0), qs::kFuseMax, 4));
  }

  // P bounded by the depth: at depth 4, seven sets never wrap (step 4 is a new set, not outs[0]);
  // four sets at depth 4 do; a group of more sets than the depth allows does not
  {
    qs::FuseGroup g;
    CHECK(grow(g, A, 4, 4));
    CHECK(!g.can_append(A.set(4), 4));
    CHECK(!g.can_wrap(A.set(4), 4, kMax));
    CHECK(g.can_wrap(A.set(0), 4, kMax));
    CHECK(!g.can_wrap(A.set(0), 3, kMax));
    CHECK(!g.can_wrap(A.set(0), 1, kMax));
    qs::FuseGroup w;
    CHECK(grow(w, A, qs::kFuseMax, qs::kFuseMax + 8));   // (the depth is capped at kFuseMax)
    CHECK(!w.can_append(A.set(qs::kFuseMax), qs::kFuseMax + 8));
    CHECK(w.can_wrap(A.set(0), qs::kFuseMax + 8, kMax));
    qs::FuseGroup one;
    CHECK(grow(one, A, 1, 1));
    CHECK(!one.can_wrap(A.set(0), 1, kMax));
  }

  // ring_shape_ok: hot_shape_ok over the P distinct sets, plus a wrap, within the cap
  {
    const std::vector<unsigned> masks(qs::kFuseMax + 1, qs::kHotOutMask);
    for (int P : {2, 3, qs::kFuseMax}) {
      CHECK(qs::ring_shape_ok(flagship(), masks.data(), P, P + 1));
      CHECK(qs::ring_shape_ok(flagship(), masks.data(), P, qs::kRingMaxSteps));
      CHECK(!qs::ring_shape_ok(flagship(), masks.data(), P, P));   // no wrap: the hot instance's launch
      CHECK(!qs::ring_shape_ok(flagship(), masks.data(), P, P - 1));
      CHECK(!qs::ring_shape_ok(flagship(), masks.data(), P, qs::kRingMaxSteps + 1));
    }
    CHECK(!qs::ring_shape_ok(flagship(), masks.data(), 1, 5));
    CHECK(!qs::ring_shape_ok(flagship(), masks.data(), qs::kFuseMax + 1, 100));
    CHECK(!qs::ring_shape_ok(flagship(), nullptr, 3, 7));
    { qs::HotShape s = flagship(); s.D = 4; s.EPB = 16; CHECK(!qs::ring_shape_ok(s, masks.data(), 3, 7)); }
    { qs::HotShape s = flagship(); s.E = 12; CHECK(!qs::ring_shape_ok(s, masks.data(), 3, 7)); }
    { qs::HotShape s = flagship(); s.act_type = 2; CHECK(!qs::ring_shape_ok(s, masks.data(), 3, 7)); }
    { qs::HotShape s = flagship(); s.obs_pipe = false; CHECK(!qs::ring_shape_ok(s, masks.data(), 3, 7)); }
    std::vector<unsigned> m = masks;
    m[2] |= 16u;   // one set of the ring with terminal_obs
    CHECK(!qs::ring_shape_ok(flagship(), m.data(), 3, 7));
    CHECK(qs::ring_shape_ok(flagship(), m.data(), 2, 7));
  }
  std::printf("step_ring ok\n");
  return 0;
}
