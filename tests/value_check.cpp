// Stand-alone host check of csrc/value_sizes.h (no GPU, no HIP): the discount
// table, the byte sizes of the value tail's buffers with the 32-bit-offset bounds at
// their last accepted and first refused values, the row tile, grid and LDS plan of
// the launch, and every refusal of a value spec.
// Built and run by tests/test_value_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "value_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  // ---- the discount table: disc[0] = 1, disc[j] = disc[j - 1] · gamma, a chain of products (not pow)
  double disc[kValueMaxSteps + 1];
  value_disc(0.99, 32, disc);
  CHECK(disc[0] == 1.0 && disc[1] == 0.99 && disc[2] == 0.99 * 0.99);
  double chain = 1.0;
  for (int j = 1; j <= 32; ++j) {
    chain = chain * 0.99;
    CHECK(disc[j] == chain);
  }
  value_disc(1.0, 16, disc);
  for (int j = 0; j <= 16; ++j) CHECK(disc[j] == 1.0);
  value_disc(0.5, 7, disc);
  CHECK(disc[7] == 1.0 / 128.0);
  value_disc(0.9, 1, disc);   // n = 1 writes two entries and no more
  CHECK(disc[0] == 1.0 && disc[1] == 0.9 && disc[2] == 0.25);
  CHECK(!value_discounts(1.0) && value_discounts(0.99));

  // ---- sizes.  n = 16, C = 4 096, E = 1, D = 8, O = 27, fp32
  uint64_t b[kValueBufs];
  CHECK(value_sizes(ValueShape{16, 4096, 1, 8, 27, 4}, true, true, b));
  CHECK(b[kValueLastObs] == 4096ull * 216 * 4 && b[kValueOut] == 4096u * 4 && b[kValueRewards] == 16ull * 4096 * 4);
  CHECK(value_sizes(ValueShape{16, 4096, 1, 8, 27, 8}, true, false, b));
  CHECK(b[kValueLastObs] == 4096ull * 216 * 4 && b[kValueOut] == 4096u * 4 && b[kValueRewards] == 0);
  CHECK(value_sizes(ValueShape{7, 33, 5, 5, 38, 8}, false, true, b));
  CHECK(b[kValueLastObs] == 0 && b[kValueOut] == 0 && b[kValueRewards] == 7ull * 165 * 8);
  CHECK(value_sizes(ValueShape{7, 33, 5, 5, 38, 8}, false, false, b));
  CHECK(b[kValueLastObs] == 0 && b[kValueOut] == 0 && b[kValueRewards] == 0);
  // the horizon, the precision and empty axes
  CHECK(!value_sizes(ValueShape{0, 4, 1, 8, 27, 4}, true, true, b) && value_sizes(ValueShape{1, 4, 1, 8, 27, 4}, true, true, b));
  CHECK(value_sizes(ValueShape{32, 4, 1, 8, 27, 4}, true, true, b) && !value_sizes(ValueShape{33, 4, 1, 8, 27, 4}, true, true, b));
  CHECK(!value_sizes(ValueShape{8, 4, 1, 8, 27, 2}, true, true, b) && !value_sizes(ValueShape{8, 4, 1, 8, 27, 16}, true, true, b));
  CHECK(!value_sizes(ValueShape{8, 0, 1, 8, 27, 4}, true, true, b) && !value_sizes(ValueShape{8, 4, 0, 8, 27, 4}, true, true, b));
  CHECK(!value_sizes(ValueShape{8, 4, 1, 0, 27, 4}, true, true, b) && !value_sizes(ValueShape{8, 4, 1, 8, 0, 4}, true, true, b));
  CHECK(!value_sizes(ValueShape{8, -4, 1, 8, 27, 4}, true, true, b));
  // the 32-bit offsets.  last_obs: V · I · 4 bytes below 2^31 (I = 216: V up to 2 485 513)
  CHECK(value_sizes(ValueShape{8, 2485513, 1, 8, 27, 4}, true, false, b) && b[kValueLastObs] == 2485513ull * 864);
  CHECK(!value_sizes(ValueShape{8, 2485514, 1, 8, 27, 4}, true, false, b));
  CHECK(value_sizes(ValueShape{8, 2485514, 1, 8, 27, 4}, false, true, b));          // no net: no last_obs to index
  CHECK(value_sizes(ValueShape{8, 1 << 19, 1, 1, 1023, 4}, true, false, b));        // 2^19 · 1 023 · 4 < 2^31
  CHECK(!value_sizes(ValueShape{8, 1 << 19, 1, 1, 1024, 4}, true, false, b));       // = 2^31
  // a step of rewards: V · real_bytes below 2^31
  CHECK(value_sizes(ValueShape{8, (1 << 29) - 1, 1, 1, 1, 4}, false, true, b) && !value_sizes(ValueShape{8, 1 << 29, 1, 1, 1, 4}, false, true, b));
  CHECK(value_sizes(ValueShape{8, (1 << 28) - 1, 1, 1, 1, 8}, false, true, b) && !value_sizes(ValueShape{8, 1 << 28, 1, 1, 1, 8}, false, true, b));
  CHECK(value_sizes(ValueShape{8, 1 << 28, 1, 1, 1, 8}, false, false, b));
  // V itself, and factors that would wrap a 64-bit product
  CHECK(!value_sizes(ValueShape{8, 1 << 16, 1 << 15, 1, 1, 4}, false, false, b));
  CHECK(!value_sizes(ValueShape{8, int64_t(1) << 40, int64_t(1) << 40, 1, 1, 4}, false, false, b));
  CHECK(!value_sizes(ValueShape{8, 4, 1, int64_t(1) << 40, int64_t(1) << 40, 4}, true, false, b));

  // ---- the launch plan: tile, grid, LDS
  CHECK(value_row_tile(64, 1) == 16 && value_row_tile(64, 4096) == 16 && value_row_tile(64, 4097) == 32);
  CHECK(value_row_tile(128, 4096) == 16 && value_row_tile(128, 4097) == 32 && value_row_tile(256, 1 << 20) == 16);
  for (int N : {64, 128, 256}) {
    for (int64_t V : {int64_t(1), int64_t(5000)}) {
      const int tile = value_row_tile(N, V);
      // grids at V = 1, tile - 1, tile, tile + 1 (the plan's tile is that of its own V)
      CHECK(value_plan(N, 54, 1).grid == 1 && value_plan(N, 54, 1).tile == 16);
      CHECK(value_plan(N, 54, 15).grid == 1 && value_plan(N, 54, 16).grid == 1 && value_plan(N, 54, 17).grid == 2);
      const ValuePlan big = value_plan(N, 54, 8192 + tile + 1);
      CHECK(big.tile == (N <= 128 ? 32 : 16) && big.grid == (uint32_t)((8192 + tile + 1 + big.tile - 1) / big.tile));
      if (N <= 128) {
        CHECK(value_plan(N, 54, 8192 + 31).grid == 257 && value_plan(N, 54, 8192 + 32).grid == 257 &&
              value_plan(N, 54, 8192 + 33).grid == 258);
      }
      // the LDS plan within the limit for every N at I = 1, 54 and 1 024, whatever the tile
      for (int I : {1, 54, 1024}) {
        const ValuePlan p = value_plan(N, I, V);
        CHECK(p.tile == tile && p.fits && p.lds_bytes <= kValueLdsLimit && p.lds_bytes == p.lds_h + p.lds_w + p.lds_x);
        CHECK(p.lds_h == (uint32_t)tile * (N + 2) * 4 && p.lds_w == (uint32_t)N * 34 * 4 && p.lds_x == (uint32_t)tile * 34 * 4);
        CHECK(p.chunks1 == (I + 31) / 32 && p.chunks2 == N / 32);
        CHECK(p.chunks1 * kValueChunk >= I && (p.chunks1 - 1) * kValueChunk < I);
      }
    }
  }
  CHECK(value_plan(256, 216, 4096).lds_bytes == 53504 && value_plan(64, 216, 4096).lds_bytes == 15104);
  CHECK(value_plan(128, 216, 5000).lds_bytes == 38400);
  // the kernel's assumptions: whole row tiles of the MFMA, a chunk of whole k-steps, a stride of 2 mod 32 banks,
  // one column tile per wave at least, eight lanes a row in the last sum
  CHECK(kValueChunk % kValueMfmaK == 0 && (kValueChunk + kValuePad) % 32 == 2 && (64 + kValuePad) % 32 == 2);
  CHECK(64 / (kValueWaves * kValueMfmaM) == 1 && 2 * kValueMfmaM * 8 <= kValueThreads && kValueThreads == 8 * kValueChunk);
  CHECK(value_plan(256, 1024, (int64_t(1) << 31) - 1).grid == (1u << 27));
  CHECK(value_fold_grid(1) == 1 && value_fold_grid(256) == 1 && value_fold_grid(257) == 2);

  // ---- refusals, in the order of the checks
  const ValueShape sh{16, 64, 5, 8, 27, 4};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  ValueSpecShape ok{216, 64, 6, true, true, 1e-8, 10.0, 0.99, 1.0};
  CHECK(value_refusal(ok, sh, false) == kValueOk);
  CHECK(value_refusal(ok, sh, true) == kValuePerDrone);
  ValueSpecShape v = ok;
  for (int k = 1; k <= 5; ++k) { v.net_ptrs = k; CHECK(value_refusal(v, sh, false) == kValuePartNet); }
  v = ok; v.in_dim = 215; CHECK(value_refusal(v, sh, false) == kValueInDim);
  v = ok; v.in_dim = 0; CHECK(value_refusal(v, sh, false) == kValueInDim);
  v = ok; v.in_dim = 1024; CHECK(value_refusal(v, ValueShape{16, 64, 5, 32, 32, 4}, false) == kValueOk);
  v = ok; v.in_dim = 1025; CHECK(value_refusal(v, ValueShape{16, 64, 5, 25, 41, 4}, false) == kValueInDim);
  v = ok; v.in_dim = 1056; CHECK(value_refusal(v, ValueShape{16, 64, 5, 32, 33, 4}, false) == kValueInDim);
  for (int N : {0, 32, 63, 65, 96, 192, 257, 512}) { v = ok; v.hidden = N; CHECK(value_refusal(v, sh, false) == kValueHidden); }
  for (int N : {64, 128, 256}) { v = ok; v.hidden = N; CHECK(value_refusal(v, sh, false) == kValueOk); }
  v = ok; v.mean = false; CHECK(value_refusal(v, sh, false) == kValuePartNorm);
  v = ok; v.var = false; CHECK(value_refusal(v, sh, false) == kValuePartNorm);
  v = ok; v.mean = v.var = false; CHECK(value_refusal(v, sh, false) == kValueOk);
  v = ok; v.net_ptrs = 0; CHECK(value_refusal(v, sh, false) == kValueNormNoNet);
  v = ok; v.eps = -1.0; CHECK(value_refusal(v, sh, false) == kValueNormArgs);
  v = ok; v.clip = 0.0; CHECK(value_refusal(v, sh, false) == kValueNormArgs);
  v = ok; v.clip = nan; CHECK(value_refusal(v, sh, false) == kValueNormArgs);
  for (double g : {0.0, -0.5, 1.0000001, inf, nan}) { v = ok; v.gamma = g; CHECK(value_refusal(v, sh, false) == kValueGamma); }
  v = ok; v.gamma = 1.0; CHECK(value_refusal(v, sh, false) == kValueOk);
  v = ok; v.gamma = 1e-300; CHECK(value_refusal(v, sh, false) == kValueOk);
  for (double s : {inf, -inf, nan}) { v = ok; v.scale = s; CHECK(value_refusal(v, sh, false) == kValueScale); }
  v = ok; v.scale = -2.5; CHECK(value_refusal(v, sh, false) == kValueOk);
  v = ok; v.scale = 0.0; CHECK(value_refusal(v, sh, false) == kValueOk);
  CHECK(value_refusal(ok, ValueShape{16, 2485513, 1, 8, 27, 4}, false) == kValueOk);
  CHECK(value_refusal(ok, ValueShape{16, 2485514, 1, 8, 27, 4}, false) == kValueOffsets);   // last_obs past 2^31 bytes
  // discount only (no net): in_dim and hidden are not read, there is no last_obs to index
  ValueSpecShape none{0, 0, 0, false, false, 0.0, 0.0, 0.99, 1.0};
  CHECK(value_refusal(none, sh, false) == kValueOk && value_refusal(none, sh, true) == kValuePerDrone);
  CHECK(value_refusal(none, ValueShape{16, 2485514, 1, 8, 27, 4}, false) == kValueOk);
  none.gamma = 1.0;
  CHECK(value_refusal(none, sh, false) == kValueOk && !value_has_net(none) && value_has_net(ok));
  std::printf("value_sizes ok\n");
  return 0;
}
