// Stand-alone host check of qs::obs_pipe_ok (csrc/step_fuse.h; no GPU, no HIP):
// which multi-step launches may take the kernel's fast obs path.  Built and run
// by tests/test_step_pipe_host.py with -fsanitize=address,undefined.
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
  using qs::obs_pipe_ok;
  // C3: 8 envs × 8 drones per workgroup, 27 floats a row
  const int rows = 64, O = 27;
  alignas(64) static float mem[qs::kFuseMax * 64 + 8];
  std::vector<const void*> obs(qs::kFuseMax);
  for (int j = 0; j < qs::kFuseMax; ++j) obs[j] = mem + 64 * j;   // 256-byte steps: aligned

  CHECK(obs_pipe_ok(true, 64, rows, O, obs.data(), qs::kFuseMax));
  CHECK(obs_pipe_ok(true, 64, rows, O, obs.data(), 1));
  CHECK(obs_pipe_ok(true, 100, rows, O, obs.data(), 2));           // more stage than rows

  // misaligned: every step, one step (first, middle, last), by 4 / 8 / 12 bytes
  for (int off = 1; off < 4; ++off) {
    std::vector<const void*> m = obs;
    for (auto& p : m) p = (const float*)p + off;
    CHECK(!obs_pipe_ok(true, 64, rows, O, m.data(), qs::kFuseMax));
    for (int j : {0, 13, qs::kFuseMax - 1}) {
      m = obs;
      m[j] = (const float*)m[j] + off;
      CHECK(!obs_pipe_ok(true, 64, rows, O, m.data(), qs::kFuseMax));
      CHECK(obs_pipe_ok(true, 64, rows, O, m.data(), j));   // the steps before it alone are fine
    }
  }
  {   // a misaligned pointer past the launch's steps is not looked at
    std::vector<const void*> m = obs;
    m[5] = (const char*)m[5] + 1;
    CHECK(obs_pipe_ok(true, 64, rows, O, m.data(), 5) && !obs_pipe_ok(true, 64, rows, O, m.data(), 6));
  }

  // null obs: a step without obs is free, so is a launch without any
  {
    std::vector<const void*> m = obs;
    for (int j = 1; j < qs::kFuseMax; j += 2) m[j] = nullptr;
    CHECK(obs_pipe_ok(true, 64, rows, O, m.data(), qs::kFuseMax));
    std::vector<const void*> none(qs::kFuseMax, nullptr);
    CHECK(obs_pipe_ok(true, 64, rows, O, none.data(), qs::kFuseMax));
    m[2] = (const float*)obs[2] + 1;
    CHECK(!obs_pipe_ok(true, 64, rows, O, m.data(), qs::kFuseMax));
  }

  // multi-pass staging (fewer staged rows than the workgroup has)
  CHECK(!obs_pipe_ok(true, 63, rows, O, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 1, rows, O, obs.data(), 4));
  // run-time control frequency
  CHECK(!obs_pipe_ok(false, 64, rows, O, obs.data(), 4));
  // row counts whose span is not a whole number of float4 (63 × 27, 62 × 27 floats), and one whose span
  // is (12 envs of 5 drones) but leaves lanes of the wave idle: only a full wave of rows takes the path
  CHECK(!obs_pipe_ok(true, 64, 63, O, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 64, 62, O, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 64, 60, O, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 128, 128, O, obs.data(), 4));
  // rows wider than the kernel keeps in flight; degenerate shapes
  CHECK(obs_pipe_ok(true, 64, rows, qs::kObsPipeMaxRow, obs.data(), 4));
  CHECK(obs_pipe_ok(true, 64, rows, 1, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 64, rows, qs::kObsPipeMaxRow + 1, obs.data(), 4));
  CHECK(!obs_pipe_ok(true, 64, 0, O, obs.data(), 4) && !obs_pipe_ok(true, 64, rows, 0, obs.data(), 4));
  CHECK(obs_pipe_ok(true, 64, rows, O, obs.data(), 0));   // no steps: nothing to refuse
  std::printf("step_pipe ok\n");
  return 0;
}
