// Stand-alone host check of csrc/step_fuse.h's SeqGroup and seq_depth_cap (no
// GPU, no HIP): which steps of an action sequence may share a launch, and how
// many action rows a launch may hold in LDS.  Built and run by
// tests/test_step_seq_host.py with -fsanitize=address,undefined.
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

int main() {
  using qs::FuseOuts;
  using qs::SeqGroup;
  // obs, reward, terminated, truncated, terminal_obs, reasons, actions_out; an action buffer is 16 bytes
  const size_t sizes[qs::kFuseOuts] = {64, 8, 2, 2, 64, 4, 16};
  const size_t act = 16;
  // a slot: the outputs, 16 free bytes, the actions, 16 free bytes
  const size_t pad = 16;
  size_t outs_bytes = 0;
  for (size_t b : sizes) outs_bytes += b;
  const size_t slot = outs_bytes + pad + act + pad;
  const int nslots = 40;
  std::vector<unsigned char> mem(slot * nslots);
  auto outs = [&](int k) {   // the 7 disjoint output buffers of slot k
    FuseOuts o{};
    unsigned char* p = mem.data() + slot * (size_t)k;
    for (int i = 0; i < qs::kFuseOuts; ++i) { o.p[i] = p; p += sizes[i]; }
    return o;
  };
  auto acts = [&](int k) -> const unsigned char* { return mem.data() + slot * (size_t)k + outs_bytes + pad; };
  auto at = [](const void* p, long off) -> const unsigned char* { return (const unsigned char*)p + off; };

  // depth: as FuseGroup (1 never joins, never past the depth or kFuseMax)
  SeqGroup g;
  CHECK(!g.can_append(outs(0), acts(0), 16));   // not begun
  g.begin(sizes, outs(0), acts(0), act);
  CHECK(g.count() == 1 && !g.can_append(outs(1), acts(1), 1));
  for (int k = 1; k < 4; ++k) {
    CHECK(g.can_append(outs(k), acts(k), 4));
    g.append(outs(k), acts(k));
  }
  CHECK(g.count() == 4 && !g.can_append(outs(4), acts(4), 4) && g.can_append(outs(4), acts(4), 16));
  for (int k = 4; k < qs::kFuseMax; ++k) {
    CHECK(g.can_append(outs(k), acts(k), 1000));
    g.append(outs(k), acts(k));
  }
  CHECK(g.count() == qs::kFuseMax && !g.can_append(outs(35), acts(35), 1000));   // full: acts[] is never overrun
  CHECK(g.acts[qs::kFuseMax - 1] == acts(qs::kFuseMax - 1));

  // shared action buffers: every step reads slot 0's, or overlapping ranges
  g.begin(sizes, outs(0), acts(0), act);
  CHECK(g.can_append(outs(1), acts(0), 16));
  g.append(outs(1), acts(0));
  CHECK(g.can_append(outs(2), at(acts(0), 4), 16) && g.can_append(outs(2), at(acts(0), -4), 16));
  g.begin(sizes, outs(0), acts(0), act);
  g.append(outs(1), acts(1));
  // the output rule of FuseGroup still holds
  CHECK(!g.can_append(outs(1), acts(2), 16));

  // direction 1: the new step's actions against the outputs of steps in the group
  CHECK(!g.can_append(outs(2), outs(0).p[6], 16));          // reads what step 0 wrote as actions_out
  CHECK(!g.can_append(outs(2), outs(1).p[0], 16));          // the head of step 1's obs
  CHECK(!g.can_append(outs(2), at(outs(1).p[0], 60), 16));  // 4 bytes into the tail of step 1's obs
  CHECK(!g.can_append(outs(2), at(outs(0).p[1], -12), 16)); // reaches 4 bytes into step 0's reward
  // ranges that touch without overlapping
  CHECK(g.can_append(outs(2), at(outs(1).p[6], 16), 16));   // begins where step 1's actions_out ends
  CHECK(g.can_append(outs(2), at(outs(1).p[0], -16), 16));  // ends where step 1's obs begins

  // direction 2: the new step's outputs against the actions of steps in the group
  FuseOuts o = outs(2);
  o.p[1] = at(acts(1), 8);                  // reward is a view into step 1's actions
  CHECK(!g.can_append(o, acts(2), 16));
  o = outs(2);
  o.p[5] = at(acts(0), 14);                 // reasons begin 2 bytes before step 0's actions end
  CHECK(!g.can_append(o, acts(2), 16));
  o = outs(2);
  o.p[6] = acts(0);                         // actions_out over step 0's actions
  CHECK(!g.can_append(o, acts(2), 16));
  o = outs(2);
  o.p[3] = at(acts(1), 16);                 // truncated begins where step 1's actions end
  CHECK(g.can_append(o, acts(2), 16));
  o = outs(2);
  o.p[3] = at(acts(1), -2);                 // truncated ends where they begin
  CHECK(g.can_append(o, acts(2), 16));
  // a step's own actions against its own outputs are the single step's business
  o = outs(2);
  o.p[6] = acts(2);
  CHECK(g.can_append(o, acts(2), 16));

  // null outputs: free in both directions (a null pointer is no range at address 0)
  FuseOuts none{};
  CHECK(g.can_append(none, acts(2), 16));
  SeqGroup h;
  h.begin(sizes, none, acts(0), act);
  CHECK(h.can_append(none, acts(0), 16) && h.can_append(outs(3), acts(3), 16));
  h.append(none, acts(1));
  CHECK(h.can_append(outs(0), acts(5), 16));
  o = outs(5);
  o.p[2] = acts(1);
  CHECK(!h.can_append(o, acts(5), 16));

  // the later step of the aliasing pairs, seen from the other side: step j's reward is a
  // view into the action buffer of a LATER step: the later step is the one refused
  g.begin(sizes, outs(0), acts(0), act);
  o = outs(1);
  o.p[1] = at(acts(3), 4);
  g.append(o, acts(1));
  CHECK(g.can_append(outs(2), acts(2), 16));
  g.append(outs(2), acts(2));
  CHECK(!g.can_append(outs(3), acts(3), 16));

  // ---- seq_depth_cap: kSeqStepBytes · A bytes per step
  using qs::seq_depth_cap;
  const size_t B = qs::kSeqStepBytes;
  CHECK(B == 256);
  CHECK(seq_depth_cap(32 * B, 64 * B, 1, 32) == 32);
  CHECK(seq_depth_cap(32 * B - 1, 64 * B, 1, 32) == 31);        // whole rows only
  CHECK(seq_depth_cap(1000 * B, 1000 * B, 1, 1000) == qs::kFuseMax);
  CHECK(seq_depth_cap(1000 * B, 1000 * B, 4, 16) == 16);        // the handle's depth
  CHECK(seq_depth_cap(1000 * B, 1000 * B, 4, 1) == 1 && seq_depth_cap(1000 * B, 1000 * B, 4, 0) == 1);
  CHECK(seq_depth_cap(19 * B, 100 * B, 1, 32) == 19);           // residency before depth
  CHECK(seq_depth_cap(19 * B, 100 * B, 4, 32) == 4);            // 4 rows of A = 4 fit the share
  CHECK(seq_depth_cap(19 * B, 100 * B, 3, 32) == 6);
  // fewer than kSeqMinDepth in the share: that many from the whole CU's, where they fit
  CHECK(qs::kSeqMinDepth == 4);
  CHECK(seq_depth_cap(3 * B, 100 * B, 1, 32) == 4);
  CHECK(seq_depth_cap(0, 100 * B, 4, 32) == 4);
  CHECK(seq_depth_cap(0, 100 * B, 4, 2) == 2);
  CHECK(seq_depth_cap(0, 11 * B, 4, 32) == 2);
  CHECK(seq_depth_cap(0, 3 * B, 4, 32) == 1);                   // no room at all: single steps
  CHECK(seq_depth_cap(0, 0, 1, 32) == 1);
  CHECK(seq_depth_cap(5 * B, 0, 1, 32) == 5);
  std::printf("step_seq ok\n");
  return 0;
}
