// value_sizes.h — host-side arithmetic of the value tail (qs_value_tail,
// qs_value_mppi_set / qs_value_cem_set; plain C++, no HIP).
//
// The tail runs a tanh MLP with two hidden layers of N units over the V = C · E
// rows of I = D · O floats a branch rollout left as its last obs, and folds the
// result into the rollout's return.  What is plain arithmetic lives here: which
// specs are refused, the bytes of the three buffers a planner owns for it, the
// row tile, grid and LDS plan of the launch per (N, I, V), the discount table,
// and the 32-bit-offset checks.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "planner_sizes.h"

namespace qs {

constexpr int kValueMaxIn = 1024;          // I at most
constexpr int kValueThreads = 256;         // the launch's workgroup: four waves
constexpr int kValueWaves = kValueThreads / 64;
constexpr int kValueMfmaM = 16;            // v_mfma_f32_16x16x4_f32: 16 rows, 16 columns, k = 4
constexpr int kValueMfmaK = 4;
constexpr int kValueChunk = 32;            // K-chunk: columns of X / W1 / W2 staged in LDS at a time
constexpr int kValuePad = 2;               // floats added to an LDS row: strides of 2 mod 32 banks, so the 16 rows x 2
                                           // k of a 32-lane operand read touch 32 different banks
constexpr int kValueMaxSteps = kMppiMaxSteps;   // n at most (the kernel's reward pointers and discount table)
constexpr uint32_t kValueLdsLimit = 64u * 1024u;   // static LDS of a workgroup
constexpr int kValueCUs = 256;
constexpr int kValueWideMaxHidden = 128;   // the 32-row tile is planned for N <= 128 only (LDS, registers)

// The buffers a planner owns once a value is attached.
enum { kValueLastObs = 0, kValueOut, kValueRewards, kValueBufs };

inline bool value_hidden_ok(int64_t N) { return N == 64 || N == 128 || N == 256; }

// Why a value spec is refused (0: it is not).  The order is the order of the checks.
enum ValueRefusal {
  kValueOk = 0,
  kValuePerDrone,      // a per-drone planner: a centralized critic has one value per env
  kValueInDim,         // in_dim != D · O, < 1 or > kValueMaxIn (checked only with a net)
  kValueHidden,        // hidden outside {64, 128, 256} (checked only with a net)
  kValuePartNet,       // some of the six weight pointers NULL, some not
  kValuePartNorm,      // one of obs_mean / obs_var without the other
  kValueNormNoNet,     // a normaliser without a net
  kValueNormArgs,      // obs_eps / obs_clip not finite, eps < 0 or clip <= 0 (checked only with a normaliser)
  kValueGamma,         // gamma outside (0, 1]
  kValueScale,         // scale not finite
  kValueOffsets,       // last_obs, C · E · D · O · 4 bytes, past the 32-bit offsets (or a rewards step past them)
};

struct ValueSpecShape {
  int64_t in_dim, hidden;
  int net_ptrs;        // how many of w1, b1, w2, b2, w3, b3 are not NULL
  bool mean, var;      // obs_mean / obs_var not NULL
  double eps, clip, gamma, scale;
};

// The shape the tail runs over.  real_bytes: 4 or 8, the precision of the rewards.
struct ValueShape {
  int64_t n, C, E, D, O, real_bytes;
};

inline bool value_has_net(const ValueSpecShape& s) { return s.net_ptrs == 6; }
inline bool value_discounts(double gamma) { return gamma != 1.0; }

// Bytes of last_obs [C][E][D][O] f32, value [C][E] f32 (both only with a net) and
// rewards [n][C][E] reals (only with gamma != 1); 0 where a buffer does not exist.
// false where the shape is outside what the launch indexes: n outside 1 ..
// kValueMaxSteps, V = C · E not in 1 .. 2^31 - 1, or last_obs or one step of
// rewards at or past 2^31 bytes.  Every product is formed in 64 bits from factors
// bounded first.
inline bool value_sizes(const ValueShape& s, bool net, bool discounts, uint64_t b[kValueBufs]) {
  const uint64_t lim = uint64_t(1) << 31;
  if (s.n < 1 || s.n > kValueMaxSteps || s.C < 1 || s.E < 1 || s.D < 1 || s.O < 1) return false;
  if (s.real_bytes != 4 && s.real_bytes != 8) return false;
  if ((uint64_t)s.C >= lim || (uint64_t)s.E >= lim || (uint64_t)s.D >= lim || (uint64_t)s.O >= lim) return false;
  const uint64_t V = (uint64_t)s.C * (uint64_t)s.E;       // < 2^62
  if (V >= lim) return false;
  const uint64_t I = (uint64_t)s.D * (uint64_t)s.O;       // < 2^62
  if (I >= lim) return false;
  const uint64_t obs = V * I;                              // < 2^62
  if (net && obs * 4u >= lim) return false;
  if (discounts && V * (uint64_t)s.real_bytes >= lim) return false;
  b[kValueLastObs] = net ? obs * 4u : 0;
  b[kValueOut] = net ? V * 4u : 0;
  b[kValueRewards] = discounts ? (uint64_t)s.n * V * (uint64_t)s.real_bytes : 0;
  return true;
}

// The checks of a value spec against the planner it is attached to, in the order of ValueRefusal.
inline ValueRefusal value_refusal(const ValueSpecShape& v, const ValueShape& s, bool per_drone) {
  if (per_drone) return kValuePerDrone;
  if (v.net_ptrs != 0 && v.net_ptrs != 6) return kValuePartNet;
  const bool net = value_has_net(v);
  if (net) {
    if (v.in_dim < 1 || v.in_dim > kValueMaxIn || s.D < 1 || s.O < 1 || s.D > kValueMaxIn || s.O > kValueMaxIn ||
        v.in_dim != s.D * s.O)
      return kValueInDim;
    if (!value_hidden_ok(v.hidden)) return kValueHidden;
  }
  if (v.mean != v.var) return kValuePartNorm;
  if (v.mean && !net) return kValueNormNoNet;
  if (v.mean && (!std::isfinite(v.eps) || !std::isfinite(v.clip) || v.eps < 0.0 || !(v.clip > 0.0))) return kValueNormArgs;
  if (!(v.gamma > 0.0) || !(v.gamma <= 1.0)) return kValueGamma;
  if (!std::isfinite(v.scale)) return kValueScale;
  uint64_t b[kValueBufs];
  if (!value_sizes(s, net, value_discounts(v.gamma), b)) return kValueOffsets;
  return kValueOk;
}

// disc[0 .. n]: disc[0] = 1, disc[j] = disc[j - 1] · gamma, in double.  The kernel
// reads this table; nothing is formed with pow.
inline void value_disc(double gamma, int n, double* disc) {
  disc[0] = 1.0;
  for (int j = 1; j <= n; ++j) disc[j] = disc[j - 1] * gamma;
}

// The launch per (N, I, V).  A workgroup takes `tile` rows: 16, or 32 where N <=
// 128 and 16-row tiles would be more than one per compute unit (the weights are
// read once per workgroup, so the wider tile halves that traffic).  Its LDS holds
// the activations H [tile][N + pad] (H1, then H2 · w3), one K-chunk of the layer's
// weights W [N][chunk + pad] and one K-chunk of the normalised input X
// [tile][chunk + pad]: W1 and W2 are streamed through the same chunk buffer, so
// the plan does not depend on I.  chunks1 / chunks2: K-chunks of the two layers.
struct ValuePlan {
  int tile;            // rows per workgroup
  uint32_t grid;       // workgroups
  uint32_t lds_h, lds_w, lds_x, lds_bytes;
  int chunks1, chunks2;
  bool fits;           // lds_bytes <= kValueLdsLimit
};
inline int value_row_tile(int64_t N, int64_t V) {
  return (N <= kValueWideMaxHidden && V > (int64_t)kValueMfmaM * kValueCUs) ? 2 * kValueMfmaM : kValueMfmaM;
}
inline ValuePlan value_plan(int64_t N, int64_t I, int64_t V) {
  ValuePlan p;
  p.tile = value_row_tile(N, V);
  p.grid = mppi_div_up((uint64_t)V, (uint64_t)p.tile);
  p.lds_h = (uint32_t)(p.tile * (N + kValuePad) * 4);
  p.lds_w = (uint32_t)(N * (kValueChunk + kValuePad) * 4);
  p.lds_x = (uint32_t)(p.tile * (kValueChunk + kValuePad) * 4);
  p.lds_bytes = p.lds_h + p.lds_w + p.lds_x;
  p.chunks1 = (int)((I + kValueChunk - 1) / kValueChunk);
  p.chunks2 = (int)(N / kValueChunk);
  p.fits = p.lds_bytes <= kValueLdsLimit;
  return p;
}

// Grid of the fold-only launch (no net, gamma != 1): one thread per row.
inline uint32_t value_fold_grid(int64_t V) { return mppi_div_up((uint64_t)V, kValueThreads); }

}  // namespace qs
