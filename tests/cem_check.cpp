// Stand-alone host check of csrc/cem_sizes.h (no GPU, no HIP): the byte sizes of a
// CEM planner's buffers, every refusal bound at its last accepted and first
// refused value, the choice between the two select + refit variants, the index
// bytes of the select key and the launch grids.
// Built and run by tests/test_cem_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "cem_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  uint64_t b[kCemBufs];
  // ---- sizes.  n = 16, C = 4 096, K = 512, I = 3, E = 1, D = 8, A = 1
  CHECK(cem_sizes(CemShape{16, 4096, 512, 3, 1, 8, 1}, b));
  CHECK(b[kCemMean] == 16u * 8 * 4 && b[kCemStd] == 16u * 8 * 4 && b[kCemCandidates] == 16ull * 4096 * 8 * 4);
  CHECK(b[kCemRet] == 4096u * 8 && b[kCemFirstDone] == 4096u * 4);
  CHECK(b[kCemElites] == 512u * 4 && b[kCemIterBest] == 3u * 8 && b[kCemAction] == 8 * 4 && b[kCemTick] == 8);
  // A = 4, an odd env count
  CHECK(cem_sizes(CemShape{7, 9, 3, 2, 21, 3, 4}, b));
  CHECK(b[kCemMean] == 7u * 21 * 12 * 4 && b[kCemStd] == b[kCemMean] && b[kCemCandidates] == 7u * 9 * 21 * 12 * 4);
  CHECK(b[kCemRet] == 189u * 8 && b[kCemFirstDone] == 189u * 4 && b[kCemElites] == 3u * 21 * 4);
  CHECK(b[kCemIterBest] == 2u * 21 * 8 && b[kCemAction] == 21u * 48);

  // ---- refusals, each at its last accepted and first refused value
  // horizon 1 .. 32
  CHECK(!cem_sizes(CemShape{0, 4, 1, 1, 1, 8, 1}, b) && cem_sizes(CemShape{1, 4, 1, 1, 1, 8, 1}, b));
  CHECK(cem_sizes(CemShape{32, 4, 1, 1, 1, 8, 1}, b) && !cem_sizes(CemShape{33, 4, 1, 1, 1, 8, 1}, b));
  // candidates 2 .. 2^27
  CHECK(!cem_sizes(CemShape{8, 1, 1, 1, 1, 8, 1}, b) && cem_sizes(CemShape{8, 2, 1, 1, 1, 8, 1}, b));
  CHECK(!cem_sizes(CemShape{8, 0, 1, 1, 1, 8, 1}, b) && !cem_sizes(CemShape{8, -5, 1, 1, 1, 8, 1}, b));
  CHECK(cem_sizes(CemShape{32, int64_t(1) << 27, 1024, 16, 1, 1, 1}, b));
  CHECK(b[kCemCandidates] == (uint64_t(32) << 27) * 4u && b[kCemElites] == 4096 && b[kCemIterBest] == 128);
  CHECK(!cem_sizes(CemShape{32, (int64_t(1) << 27) + 1, 1024, 16, 1, 1, 1}, b));
  // elites 1 .. min(C, 1 024)
  CHECK(!cem_sizes(CemShape{8, 4, 0, 1, 1, 8, 1}, b) && cem_sizes(CemShape{8, 4, 1, 1, 1, 8, 1}, b));
  CHECK(!cem_sizes(CemShape{8, 4, -1, 1, 1, 8, 1}, b));
  CHECK(cem_sizes(CemShape{8, 4, 4, 1, 1, 8, 1}, b) && !cem_sizes(CemShape{8, 4, 5, 1, 1, 8, 1}, b));            // K = C
  CHECK(cem_sizes(CemShape{8, 1024, 1024, 1, 1, 8, 1}, b) && !cem_sizes(CemShape{8, 1024, 1025, 1, 1, 8, 1}, b));
  CHECK(cem_sizes(CemShape{8, 4096, 1024, 1, 1, 8, 1}, b) && !cem_sizes(CemShape{8, 4096, 1025, 1, 1, 8, 1}, b)); // K = 1 024 / 1 025
  // iterations 1 .. 16
  CHECK(!cem_sizes(CemShape{8, 4, 1, 0, 1, 8, 1}, b) && cem_sizes(CemShape{8, 4, 1, 1, 1, 8, 1}, b));
  CHECK(cem_sizes(CemShape{8, 4, 1, 16, 1, 8, 1}, b) && !cem_sizes(CemShape{8, 4, 1, 17, 1, 8, 1}, b));
  CHECK(kCemMaxIterations <= 256);   // the iteration has bits 8 .. 15 of the counter word
  // envs, drones, components, the row of D · A <= 256
  CHECK(!cem_sizes(CemShape{8, 4, 1, 1, 0, 8, 1}, b) && !cem_sizes(CemShape{8, 4, 1, 1, 1, 0, 1}, b));
  CHECK(!cem_sizes(CemShape{8, 4, 1, 1, 1, 8, 0}, b) && cem_sizes(CemShape{8, 4, 1, 1, 1, 8, 4}, b) &&
        !cem_sizes(CemShape{8, 4, 1, 1, 1, 8, 5}, b));
  CHECK(cem_sizes(CemShape{8, 4, 1, 1, 1, 64, 4}, b) && !cem_sizes(CemShape{8, 4, 1, 1, 1, 65, 4}, b));
  CHECK(cem_sizes(CemShape{8, 4, 1, 1, 1, 256, 1}, b) && !cem_sizes(CemShape{8, 4, 1, 1, 1, 257, 1}, b));
  // qs_score's 32-bit offsets: C · E virtual envs, C · E · D virtual agents, a step's actions, ret
  CHECK(!cem_sizes(CemShape{8, 1 << 16, 8, 3, 1 << 15, 1, 1}, b));            // C · E = 2^31
  CHECK(cem_sizes(CemShape{8, 1 << 14, 8, 3, 1 << 13, 1, 1}, b));             // 2^27 virtual envs, 2^30 B of ret
  CHECK(b[kCemElites] == 8u * 8192 * 4 && b[kCemIterBest] == 3u * 8192 * 8);
  CHECK(!cem_sizes(CemShape{8, 1 << 14, 8, 3, 1 << 14, 1, 1}, b));            // ret: 2^28 · 8 = 2^31 B
  CHECK(!cem_sizes(CemShape{8, 1 << 12, 8, 3, 1 << 12, 128, 1}, b));          // C · E · D = 2^31
  CHECK(cem_sizes(CemShape{8, 1 << 12, 8, 3, 1 << 12, 31, 1}, b));            // a step: 2^24 · 31 · 4 < 2^31 B
  CHECK(!cem_sizes(CemShape{8, 1 << 12, 8, 3, 1 << 12, 32, 1}, b));           // a step: 2^31 B
  CHECK(!cem_sizes(CemShape{8, 4, 1, 1, int64_t(1) << 31, 1, 1}, b) && !cem_sizes(CemShape{8, 4, 1, 1, 1, int64_t(1) << 62, 1}, b));

  // ---- variant.  The three measured shapes (D = 8, A = 1), then the boundaries
  CHECK(cem_variant(1, 4096, 8) == kCemPerBlock && cem_variant(64, 256, 8) == kCemPerBlock);
  CHECK(cem_variant(4096, 4, 8) == kCemPerThread);
  CHECK(cem_variant(1, 63, 8) == kCemPerThread && cem_variant(1, 64, 8) == kCemPerBlock);
  CHECK(cem_variant(2047, 64, 8) == kCemPerBlock && cem_variant(2048, 64, 8) == kCemPerThread);
  CHECK(cem_variant(4096, 511, 8) == kCemPerThread && cem_variant(4096, 512, 8) == kCemPerBlock);   // C^2 a thread: no
  CHECK(cem_variant(5, 130, 8) == kCemPerBlock && cem_variant(2, 2100, 8) == kCemPerBlock &&
        cem_variant(300, 9, 8) == kCemPerThread && cem_variant(5, 9, 12) == kCemPerThread);

  // ---- the select key's index bytes: C - 1 in 1 .. 4 bytes
  CHECK(cem_index_bytes(2) == 1 && cem_index_bytes(256) == 1 && cem_index_bytes(257) == 2);
  CHECK(cem_index_bytes(65536) == 2 && cem_index_bytes(65537) == 3 && cem_index_bytes(1 << 24) == 3);
  CHECK(cem_index_bytes((1 << 24) + 1) == 4 && cem_index_bytes(int64_t(1) << 27) == 4);
  CHECK(kCemStage * 8 + kCemMaxElites * 12 + 256 * 4 + 12 <= 64 * 1024);   // the select workgroup's LDS
  CHECK(kCemMaxElites <= kCemBlockThreads);                                // one elite per thread in the last ranking

  // ---- grids
  CemShape s{16, 4096, 512, 3, 1, 8, 1};
  CemGrids g = cem_grids(s, cem_variant(s.E, s.C, s.D * s.A));
  CHECK(g.fill == 1 && g.sample == 4096u * 8 / 256 && g.select == 1 && g.refit == 16 && g.finish == 1);
  s = CemShape{16, 256, 32, 3, 64, 8, 1};
  g = cem_grids(s, cem_variant(s.E, s.C, s.D * s.A));
  CHECK(g.fill == 16u * 64 * 8 / 256 && g.sample == 256u * 64 * 8 / 256 && g.select == 64 && g.refit == 1024 && g.finish == 2);
  s = CemShape{16, 4, 1, 3, 4096, 8, 1};
  g = cem_grids(s, cem_variant(s.E, s.C, s.D * s.A));
  CHECK(g.fill == 16u * 4096 * 8 / 256 && g.sample == 4u * 4096 * 8 / 256 && g.select == 16 && g.refit == g.fill &&
        g.finish == 128);
  s = CemShape{7, 5, 2, 2, 21, 3, 4};   // tails: 7 · 21 · 12 = 1 764 elements, 315 threads a step, 21 envs, 252 columns
  g = cem_grids(s, kCemPerThread);
  CHECK(g.fill == 7 && g.sample == 2 && g.select == 1 && g.refit == 7 && g.finish == 1);
  g = cem_grids(s, kCemPerBlock);
  CHECK(g.select == 21 && g.refit == 147 && g.fill == 7 && g.finish == 1);
  s = CemShape{32, int64_t(1) << 27, 1024, 16, 1, 1, 1};   // 2^27 threads a step
  g = cem_grids(s, kCemPerBlock);
  CHECK(g.sample == (1u << 19) && g.refit == 32 && g.select == 1);
  std::printf("cem_sizes ok\n");
  return 0;
}
