// Stand-alone host check of csrc/prior_sizes.h (no GPU, no HIP): every refusal of a
// prior spec, the byte sizes of the prior's buffers with the 32-bit-offset bounds at
// their last accepted and first refused values, the row tile, grid and LDS plan of
// the actor launch for each hidden size, the inject grid, and K = 1 and K = C - 1.
// Built and run by tests/test_prior_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "prior_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  CHECK(kPriorTag == 7 && kPriorTag != kMppiTag && kPriorMaxAct == 4 && kPriorMaxDrones <= 256);

  // ---- sizes.  n = 16, K = 4, C = 4 096, E = 1, D = 8, O = 27, A = 1
  uint64_t b[kPriorBufs];
  CHECK(prior_sizes(PriorShape{16, 4, 4096, 1, 8, 27, 1}, b));
  CHECK(b[kPriorActions] == 16ull * 4 * 8 * 4 && b[kPriorObs] == 16ull * 4 * 8 * 27 * 4);
  CHECK(prior_sizes(PriorShape{7, 3, 8, 5, 2, 38, 3}, b));
  CHECK(b[kPriorActions] == 7ull * 30 * 3 * 4 && b[kPriorObs] == 7ull * 30 * 38 * 4);
  // the horizon and empty axes
  CHECK(!prior_sizes(PriorShape{0, 4, 8, 1, 8, 27, 1}, b) && prior_sizes(PriorShape{1, 4, 8, 1, 8, 27, 1}, b));
  CHECK(prior_sizes(PriorShape{32, 4, 8, 1, 8, 27, 1}, b) && !prior_sizes(PriorShape{33, 4, 8, 1, 8, 27, 1}, b));
  CHECK(!prior_sizes(PriorShape{8, 0, 8, 1, 8, 27, 1}, b) && !prior_sizes(PriorShape{8, 4, 8, 0, 8, 27, 1}, b));
  CHECK(!prior_sizes(PriorShape{8, 4, 8, 1, 0, 27, 1}, b) && !prior_sizes(PriorShape{8, 4, 8, 1, 8, 0, 1}, b));
  CHECK(!prior_sizes(PriorShape{8, 4, 8, 1, 8, 27, 0}, b) && !prior_sizes(PriorShape{8, -4, 8, 1, 8, 27, 1}, b));
  // what the kernel's counter word and its four normals hold
  CHECK(prior_sizes(PriorShape{8, 4, 8, 1, 256, 27, 1}, b) && !prior_sizes(PriorShape{8, 4, 8, 1, 257, 27, 1}, b));
  CHECK(prior_sizes(PriorShape{8, 4, 8, 1, 8, 1024, 1}, b) && !prior_sizes(PriorShape{8, 4, 8, 1, 8, 1025, 1}, b));
  CHECK(prior_sizes(PriorShape{8, 4, 8, 1, 8, 27, 4}, b) && !prior_sizes(PriorShape{8, 4, 8, 1, 8, 27, 5}, b));
  // the 32-bit offsets.  a step's obs: R · O · 4 bytes below 2^31 (D = 8, O = 27: K · E up to 2 485 513)
  CHECK(prior_sizes(PriorShape{8, 2485513, 1 << 27, 1, 8, 27, 1}, b) && b[kPriorObs] == 8ull * 2485513 * 864);
  CHECK(!prior_sizes(PriorShape{8, 2485514, 1 << 27, 1, 8, 27, 1}, b));
  CHECK(prior_sizes(PriorShape{8, 1, 2, 2485513, 8, 27, 1}, b) && !prior_sizes(PriorShape{8, 1, 2, 2485514, 8, 27, 1}, b));
  CHECK(prior_sizes(PriorShape{8, 1 << 19, 1 << 20, 1, 1, 1023, 1}, b));           // 2^19 · 1 023 · 4 < 2^31
  CHECK(!prior_sizes(PriorShape{8, 1 << 19, 1 << 20, 1, 1, 1024, 1}, b));          // = 2^31
  // a step's actions: R · A · 4 bytes below 2^31 (O = 1, A = 4: the actions are the larger)
  CHECK(prior_sizes(PriorShape{8, (1 << 27) - 1, 1 << 27, 1, 1, 1, 4}, b) && !prior_sizes(PriorShape{8, 1 << 27, 1 << 28, 1, 1, 1, 4}, b));
  // R itself, and factors that would wrap a 64-bit product
  CHECK(!prior_sizes(PriorShape{8, 1 << 16, 1 << 17, 1 << 15, 1, 1, 1}, b));
  CHECK(!prior_sizes(PriorShape{8, int64_t(1) << 40, int64_t(1) << 41, int64_t(1) << 40, 1, 1, 1}, b));
  CHECK(!prior_sizes(PriorShape{8, 4, 8, 1, int64_t(1) << 40, int64_t(1) << 40, 1}, b));

  // ---- the launch plan: the value tail's tile, grid and LDS, over R rows of O columns
  for (int N : {64, 128, 256}) {
    for (int64_t R : {int64_t(1), int64_t(5000)}) {
      const int tile = value_row_tile(N, R);
      CHECK(prior_plan(N, 27, 1).grid == 1 && prior_plan(N, 27, 1).tile == 16);
      CHECK(prior_plan(N, 27, 16).grid == 1 && prior_plan(N, 27, 17).grid == 2);
      CHECK(prior_plan(N, 27, 4096).tile == 16 && prior_plan(N, 27, 4097).tile == (N <= 128 ? 32 : 16));
      for (int O : {1, 13, 27, 38, 1024}) {
        const ValuePlan p = prior_plan(N, O, R);
        CHECK(p.tile == tile && p.fits && p.lds_bytes <= kValueLdsLimit && p.lds_bytes == p.lds_h + p.lds_w + p.lds_x);
        CHECK(p.lds_h == (uint32_t)tile * (N + 2) * 4 && p.lds_w == (uint32_t)N * 34 * 4 && p.lds_x == (uint32_t)tile * 34 * 4);
        CHECK(p.chunks1 == (O + 31) / 32 && p.chunks2 == N / 32);
        CHECK(p.grid == (uint32_t)((R + tile - 1) / tile));
      }
    }
  }
  CHECK(prior_plan(256, 27, 4096).lds_bytes == 53504 && prior_plan(64, 27, 32).lds_bytes == 15104);
  CHECK(prior_plan(128, 27, 5000).lds_bytes == 38400 && prior_plan(64, 27, 5000).lds_bytes == 21504);
  CHECK(prior_plan(256, 1024, (int64_t(1) << 31) - 1).grid == (1u << 27));
  // the last sum takes eight lanes a row of whole waves
  CHECK(kValueMfmaM * 8 % 64 == 0 && 2 * kValueMfmaM * 8 <= kValueThreads);
  CHECK(prior_inject_grid(1, 1, 1, 1) == 1 && prior_inject_grid(4, 1, 8, 1) == 1 && prior_inject_grid(4, 4096, 8, 1) == 512);
  CHECK(prior_inject_grid(1, 257, 1, 1) == 2 && prior_inject_grid(3, 5, 2, 4) == 1);

  // ---- refusals, in the order of the checks
  const PriorShape sh{16, 4, 64, 5, 8, 27, 1};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const PriorSpecShape ok{27, 64, 1, 4, 7, true, true, true, 1e-8, 10.0, 1.0, 1.0};
  CHECK(prior_refusal(ok, sh) == kPriorOk);
  PriorSpecShape v = ok;
  for (int64_t K : {int64_t(0), int64_t(-1), int64_t(64), int64_t(65), int64_t(1) << 40}) {
    v = ok; v.count = K; CHECK(prior_refusal(v, PriorShape{16, K, 64, 5, 8, 27, 1}) == kPriorCount);
  }
  for (int64_t K : {int64_t(1), int64_t(63)}) {   // K = 1 and K = C - 1
    v = ok; v.count = K;
    const PriorShape s{16, K, 64, 5, 8, 27, 1};
    CHECK(prior_refusal(v, s) == kPriorOk && prior_sizes(s, b) && b[kPriorActions] == 16ull * K * 40 * 4 &&
          b[kPriorObs] == 16ull * K * 40 * 27 * 4);
  }
  v = ok; v.count = 1; CHECK(prior_refusal(v, PriorShape{16, 1, 2, 5, 8, 27, 1}) == kPriorOk);
  v = ok; v.count = 2; CHECK(prior_refusal(v, PriorShape{16, 2, 2, 5, 8, 27, 1}) == kPriorCount);
  for (int k = 0; k <= 6; ++k) { v = ok; v.net_ptrs = k; CHECK(prior_refusal(v, sh) == kPriorPartNet); }
  for (int N : {0, 32, 63, 65, 96, 192, 257, 512}) { v = ok; v.hidden = N; CHECK(prior_refusal(v, sh) == kPriorHidden); }
  for (int N : {64, 128, 256}) { v = ok; v.hidden = N; CHECK(prior_refusal(v, sh) == kPriorOk); }
  v = ok; v.in_dim = 26; CHECK(prior_refusal(v, sh) == kPriorInDim);
  v = ok; v.in_dim = 216; CHECK(prior_refusal(v, sh) == kPriorInDim);   // D · O is the critic's width, not the actor's
  v = ok; v.in_dim = 0; CHECK(prior_refusal(v, sh) == kPriorInDim);
  v = ok; v.in_dim = 1024; CHECK(prior_refusal(v, PriorShape{16, 4, 64, 5, 8, 1024, 1}) == kPriorOk);
  v = ok; v.in_dim = 1025; CHECK(prior_refusal(v, PriorShape{16, 4, 64, 5, 8, 1025, 1}) == kPriorInDim);
  v = ok; v.act_dim = 2; CHECK(prior_refusal(v, sh) == kPriorActDim);
  v = ok; v.act_dim = 0; CHECK(prior_refusal(v, sh) == kPriorActDim);
  v = ok; v.act_dim = 4; CHECK(prior_refusal(v, PriorShape{16, 4, 64, 5, 8, 27, 4}) == kPriorOk);
  v = ok; v.act_dim = 5; CHECK(prior_refusal(v, PriorShape{16, 4, 64, 5, 8, 27, 5}) == kPriorActDim);
  v = ok; v.mean = false; CHECK(prior_refusal(v, sh) == kPriorPartNorm);
  v = ok; v.var = false; CHECK(prior_refusal(v, sh) == kPriorPartNorm);
  v = ok; v.mean = v.var = false; v.eps = nan; v.clip = nan; CHECK(prior_refusal(v, sh) == kPriorOk);
  v = ok; v.eps = -1.0; CHECK(prior_refusal(v, sh) == kPriorNormArgs);
  v = ok; v.clip = 0.0; CHECK(prior_refusal(v, sh) == kPriorNormArgs);
  v = ok; v.clip = nan; CHECK(prior_refusal(v, sh) == kPriorNormArgs);
  v = ok; v.obs = false; CHECK(prior_refusal(v, sh) == kPriorNoObs);
  for (double s : {inf, -inf, nan, -1e-30, -1.0}) { v = ok; v.std_scale = s; CHECK(prior_refusal(v, sh) == kPriorScales); }
  for (double s : {0.0, 1e-30, 2.5}) { v = ok; v.std_scale = s; CHECK(prior_refusal(v, sh) == kPriorOk); }
  for (double s : {inf, -inf, nan}) { v = ok; v.action_scale = s; CHECK(prior_refusal(v, sh) == kPriorScales); }
  for (double s : {0.0, -0.5, 0.5}) { v = ok; v.action_scale = s; CHECK(prior_refusal(v, sh) == kPriorOk); }
  v = ok; v.count = 2485513; CHECK(prior_refusal(v, PriorShape{16, 2485513, 1 << 27, 1, 8, 27, 1}) == kPriorOk);
  v = ok; v.count = 2485514; CHECK(prior_refusal(v, PriorShape{16, 2485514, 1 << 27, 1, 8, 27, 1}) == kPriorOffsets);
  CHECK(prior_refusal(ok, PriorShape{33, 4, 64, 5, 8, 27, 1}) == kPriorOffsets);
  CHECK(prior_refusal(ok, PriorShape{16, 4, 64, 5, 257, 27, 1}) == kPriorOffsets);
  std::printf("prior_sizes ok\n");
  return 0;
}
