// Stand-alone host check of csrc/step_fuse.h (no GPU, no HIP): the record of a
// growing multi-step launch and its output-distinctness rule.  Built and run by
// tests/test_step_fuse_host.py with -fsanitize=address,undefined.
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
  using qs::FuseGroup;
  using qs::FuseOuts;
  const size_t sizes[qs::kFuseOuts] = {64, 8, 2, 2, 64, 4, 16};
  size_t slot = 0;
  for (size_t b : sizes) slot += b;
  const int nslots = 40;
  std::vector<unsigned char> mem(slot * nslots);
  auto outs = [&](int k) {   // the 7 disjoint buffers of slot k
    FuseOuts o{};
    unsigned char* p = mem.data() + slot * (size_t)k;
    for (int i = 0; i < qs::kFuseOuts; ++i) { o.p[i] = p; p += sizes[i]; }
    return o;
  };
  int stream_tag = 0, node_tag = 0, other = 0;

  FuseGroup g;
  CHECK(!g.live && !g.can_append(outs(0), 16) && !g.same_capture(0, &stream_tag));
  g.begin(sizes, outs(0), 7, &stream_tag, &node_tag);
  CHECK(g.live && g.count == 1);
  CHECK(g.same_capture(7, &stream_tag));
  CHECK(!g.same_capture(8, &stream_tag));   // another capture
  CHECK(!g.same_capture(7, &other));        // another stream
  // depth: 1 never joins; k steps at depth k, never more than kFuseMax
  CHECK(!g.can_append(outs(1), 1));
  for (int k = 1; k < 4; ++k) {
    CHECK(g.can_append(outs(k), 4));
    g.append(outs(k));
  }
  CHECK(g.count == 4 && !g.can_append(outs(4), 4) && g.can_append(outs(4), 16));
  for (int k = 4; k < qs::kFuseMax; ++k) {
    CHECK(g.can_append(outs(k), 1000));
    g.append(outs(k));
  }
  CHECK(g.count == qs::kFuseMax && !g.can_append(outs(20), 1000));   // full: outs[] is never overrun

  // distinctness: the same pointer, a partial overlap, another output's range; NULLs are free
  g.begin(sizes, outs(0));
  g.append(outs(1));
  CHECK(!g.can_append(outs(0), 16) && !g.can_append(outs(1), 16));
  FuseOuts o = outs(2);
  CHECK(g.can_append(o, 16));
  o.p[0] = (const unsigned char*)outs(1).p[0] + 60;   // obs reaches 4 bytes into slot 1's obs
  CHECK(!g.can_append(o, 16));
  o = outs(2);
  o.p[1] = (const unsigned char*)outs(0).p[0] + 8;    // reward inside slot 0's obs
  CHECK(!g.can_append(o, 16));
  o = outs(2);
  o.p[6] = (const unsigned char*)outs(1).p[6] + 16;   // begins exactly where slot 1's actions end
  o.p[5] = nullptr;
  CHECK(g.can_append(o, 16));
  FuseOuts none{};
  CHECK(g.can_append(none, 16));
  FuseGroup h;
  h.begin(sizes, none);
  CHECK(h.can_append(none, 16) && h.can_append(outs(3), 16));

  g.forget();
  CHECK(!g.live && !g.can_append(outs(5), 16) && !g.same_capture(0, nullptr));
  std::printf("step_fuse ok\n");
  return 0;
}
