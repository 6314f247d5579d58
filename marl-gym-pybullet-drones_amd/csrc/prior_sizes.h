// prior_sizes.h — host-side arithmetic of the policy prior (qs_prior_act,
// qs_prior_mppi_* / qs_prior_cem_*; plain C++, no HIP).
//
// The prior runs the trainer's actor, a tanh MLP with two hidden layers of N
// units, O inputs and A <= 4 outputs, over the R = K · E · D rows of K closed-loop
// trajectories per env, one launch per step of the horizon.  What is plain
// arithmetic lives here: which specs are refused, the bytes of the two buffers a
// planner owns for it, the 32-bit-offset checks, and the row tile, grid and LDS
// plan of the launch, which are the value tail's (value_sizes.h): the two kernels
// share the layer product and its LDS layout.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "value_sizes.h"

namespace qs {

constexpr int kPriorTag = 7;               // Philox domain tag of the prior's noise (3: MPPI, 4: CEM, 5 and 6: SMC)
constexpr int kPriorMaxAct = 4;            // A at most: the four normals of one Philox draw
constexpr int kPriorMaxDrones = kMppiMaxRow;   // D at most: the drone shares a counter word with the tag
constexpr int kPriorNetPtrs = 7;           // w1, b1, w2, b2, w3, b3, logstd

// The buffers a planner owns once a prior is attached.
enum { kPriorActions = 0, kPriorObs, kPriorBufs };

// Why a prior spec is refused (0: it is not).  The order is the order of the checks.
enum PriorRefusal {
  kPriorOk = 0,
  kPriorCount,         // count outside 1 .. C - 1 (candidate 0 stays the nominal / mean)
  kPriorPartNet,       // some of w1 .. b3, logstd NULL
  kPriorHidden,        // hidden outside {64, 128, 256}
  kPriorInDim,         // in_dim != obs_dim, < 1 or > kValueMaxIn
  kPriorActDim,        // act_dim != the swarm's, < 1 or > kPriorMaxAct
  kPriorPartNorm,      // one of obs_mean / obs_var without the other
  kPriorNormArgs,      // obs_eps / obs_clip not finite, eps < 0 or clip <= 0 (checked only with a normaliser)
  kPriorNoObs,         // obs NULL
  kPriorScales,        // std_scale not finite or negative, or action_scale not finite
  kPriorOffsets,       // n, K, E, D outside what the launch indexes, or a step's obs / actions past the 32-bit offsets
};

struct PriorSpecShape {
  int64_t in_dim, hidden, act_dim, count;
  int net_ptrs;        // how many of w1, b1, w2, b2, w3, b3, logstd are not NULL
  bool mean, var, obs; // obs_mean / obs_var / obs not NULL
  double eps, clip, action_scale, std_scale;
};

// The shape the prior runs over: n steps of K trajectories in each of E envs of D
// drones, O obs columns and A action components; C: the planner's candidates
// (qs_prior_act, bound to no planner: K + 1).
struct PriorShape {
  int64_t n, K, C, E, D, O, A;
};

// Bytes of prior_actions [n][K][E][D][A] f32 and prior_obs [n][K][E][D][O] f32.
// false where the shape is outside what the launch indexes: n outside 1 ..
// kValueMaxSteps, R = K · E · D not in 1 .. 2^31 - 1, D above kPriorMaxDrones, O
// above kValueMaxIn, A above kPriorMaxAct, or one step of obs or of actions at or
// past 2^31 bytes.  Every product is formed in 64 bits from factors bounded first.
inline bool prior_sizes(const PriorShape& s, uint64_t b[kPriorBufs]) {
  const uint64_t lim = uint64_t(1) << 31;
  if (s.n < 1 || s.n > kValueMaxSteps || s.K < 1 || s.E < 1 || s.D < 1 || s.O < 1 || s.A < 1) return false;
  if ((uint64_t)s.K >= lim || (uint64_t)s.E >= lim) return false;
  if (s.D > kPriorMaxDrones || s.O > kValueMaxIn || s.A > kPriorMaxAct) return false;
  const uint64_t V = (uint64_t)s.K * (uint64_t)s.E;        // < 2^62
  if (V >= lim) return false;
  const uint64_t R = V * (uint64_t)s.D;                    // < 2^39
  if (R >= lim) return false;
  const uint64_t obs = R * (uint64_t)s.O * 4u;             // < 2^43
  const uint64_t act = R * (uint64_t)s.A * 4u;             // < 2^35
  if (obs >= lim || act >= lim) return false;
  b[kPriorActions] = (uint64_t)s.n * act;
  b[kPriorObs] = (uint64_t)s.n * obs;
  return true;
}

// The checks of a prior spec against the shape it runs over, in the order of PriorRefusal.
inline PriorRefusal prior_refusal(const PriorSpecShape& v, const PriorShape& s) {
  if (v.count < 1 || v.count > s.C - 1) return kPriorCount;
  if (v.net_ptrs != kPriorNetPtrs) return kPriorPartNet;
  if (!value_hidden_ok(v.hidden)) return kPriorHidden;
  if (v.in_dim < 1 || v.in_dim > kValueMaxIn || v.in_dim != s.O) return kPriorInDim;
  if (v.act_dim < 1 || v.act_dim > kPriorMaxAct || v.act_dim != s.A) return kPriorActDim;
  if (v.mean != v.var) return kPriorPartNorm;
  if (v.mean && (!std::isfinite(v.eps) || !std::isfinite(v.clip) || v.eps < 0.0 || !(v.clip > 0.0))) return kPriorNormArgs;
  if (!v.obs) return kPriorNoObs;
  if (!std::isfinite(v.std_scale) || !(v.std_scale >= 0.0) || !std::isfinite(v.action_scale)) return kPriorScales;
  uint64_t b[kPriorBufs];
  if (!prior_sizes(s, b)) return kPriorOffsets;
  return kPriorOk;
}

// The actor launch per (N, O, R): the value tail's plan over R rows of O columns
// (16 rows a workgroup, or 32 where N <= 128 and 16-row tiles would be more than
// one per compute unit; the same three LDS arrays, inside the same 64 KB).
inline ValuePlan prior_plan(int64_t N, int64_t O, int64_t R) { return value_plan(N, O, R); }

// Grid x of the inject launch, a (x, n) grid of kValueThreads threads: one thread
// per float of a step's K · E · D · A prior actions.
inline uint32_t prior_inject_grid(int64_t K, int64_t E, int64_t D, int64_t A) {
  return mppi_div_up((uint64_t)K * (uint64_t)E * (uint64_t)D * (uint64_t)A, kValueThreads);
}

}  // namespace qs
