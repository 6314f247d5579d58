// planner_prior.hip — the policy prior of the MPPI and CEM ticks (include/quadswarm.h,
// qs_prior_act, qs_prior_mppi_* / qs_prior_cem_*; DESIGN.md §4a "Policy prior").
//
// K of a planner's C candidates per env are closed-loop rollouts of the trainer's
// actor from the swarm's current state.  The actor launch runs over the R = K · E · D
// rows of one step: gather the row's O floats of obs, normalise them (float64,
// the expression of qs_rms_normalize, with the trainer's [D][O] statistics), run
// pi_net on the f32-input MFMA with the activations kept in LDS (mlp_tile.h, shared
// with the value tail), form the A <= 4 outputs by lane-partial dot products,
// scale, add the policy's noise to every trajectory but the first, clip, and write
// actions[k][e][d][.] and a copy of the raw obs row.  The prior stage alternates
// that launch with one-step qs_branch_advance calls on a branch set the planner
// owns; the inject launch copies the result over the planner's last K candidates.
// Weights, logstd and statistics are read from the caller's tensors at every
// launch (no pack step).  No atomics and a fixed summation order: the same inputs
// give the same bytes.  The host arithmetic is prior_sizes.h.
#include "planner_common.h"
#include "mlp_tile.h"
#include "prior_sizes.h"

namespace {

using qs::kValueChunk;
using qs::kValueMfmaM;
using qs::kValuePad;
using qs::kValueThreads;

struct PriorParams {
  const float* x;                            // obs [R][O], or with bcast [E · D][O]
  const float *w1, *b1, *w2, *b2, *w3, *b3, *logstd;
  const double *mean, *var;                  // [D][O], or both null
  double eps, clip;
  float* actions;                            // [R][A]
  float* seen;                               // [R][O], or null
  const uint64_t* tick;
  uint32_t k0, k1, genv0, j;                 // Philox key, global id of env 0, the step
  uint32_t R, ED, D;                         // R = K · E · D rows, E · D rows a trajectory
  int O, A, bcast;
  float action_scale, std_scale, lo, hi;
};

// The obs rows as the actor takes them (mlp_tile.h, layer_product's input): row r
// is trajectory r / (E · D)'s agent r mod (E · D), read from that agent's row of
// the caller's obs where bcast is set; drone d = r mod D takes entries d · O ..
// d · O + O - 1 of the statistics.  Every raw element passes through here once, so
// this is also where the row is copied to `seen`.
struct PriorInput {
  const PriorParams& P;
  template <int XR>
  __device__ __forceinline__ void stage(size_t r0, int k, bool kv, float (&out)[XR]) const {
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const size_t r = r0 + (size_t)(8 * i);
      float xv = 0.0f;
      if (kv && r < (size_t)P.R) {
        const uint32_t r32 = (uint32_t)r, src = P.bcast ? r32 % P.ED : r32;
        xv = P.x[(size_t)src * P.O + k];
        if (P.seen) P.seen[r * (size_t)P.O + k] = xv;
        if (P.mean) {
          const size_t at = (size_t)(r32 % P.D) * P.O + k;
          xv = qs::norm1(xv, P.mean[at], sqrt(P.var[at] + P.eps), P.clip);
        }
      }
      out[i] = xv;
    }
  }
};

template <int N, int MT>
__global__ __launch_bounds__(kValueThreads) void prior_act_kernel(PriorParams P) {
  constexpr int TM = MT * kValueMfmaM, CP = kValueChunk + kValuePad, HP = N + kValuePad;
  __shared__ float sH[TM * HP];
  __shared__ float sW[N * CP];
  __shared__ float sX[TM * CP];
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * TM;
  // sH = H2 = tanh(tanh(X · W1ᵀ + b1) · W2ᵀ + b2)
  qs::hidden_layers<N, MT>(PriorInput{P}, P.O, P.w1, P.b1, P.w2, P.b2, nullptr, row0, sH, sW, sX);

  // out[a] = Σ_n H2[row][n] · w3[a][n]: eight lanes a row, each over n = part, part + 8, ..., then an xor tree
  if (tid < TM * 8) {   // (whole waves: TM · 8 is 128 or 256)
    const int row = tid >> 3, part = tid & 7;
    float s[qs::kPriorMaxAct] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int nn = part; nn < N; nn += 8) {
      const float h = sH[row * HP + nn];
#pragma unroll
      for (int a = 0; a < qs::kPriorMaxAct; ++a)
        if (a < P.A) s[a] += h * P.w3[a * N + nn];   // (kernel-uniform)
    }
#pragma unroll
    for (int a = 0; a < qs::kPriorMaxAct; ++a) {
      s[a] += __shfl_xor(s[a], 4, 64);
      s[a] += __shfl_xor(s[a], 2, 64);
      s[a] += __shfl_xor(s[a], 1, 64);
    }
    const size_t r = row0 + (size_t)row;
    if (part == 0 && r < (size_t)P.R) {
      const uint32_t r32 = (uint32_t)r, k = r32 / P.ED, ed = r32 - k * P.ED, e = ed / P.D, d = ed - e * P.D;
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (k != 0) {   // trajectory 0 is the mode; the others draw as planner_sample_kernel does
        const qs::U4 x = qs::philox(qs::U4{(uint32_t)*P.tick, P.genv0 + e, k * 32u + P.j, ((uint32_t)qs::kPriorTag << 24) | d},
                                    P.k0, P.k1);
        const float two_pi = 6.283185307179586f;
        const float r0 = sqrtf(-2.0f * logf(qs::u01_open0(x.x))), a0 = two_pi * qs::u01_open0(x.y);
        z[0] = r0 * cosf(a0);
        if (P.A > 1) z[1] = r0 * sinf(a0);
        if (P.A > 2) {   // (kernel-uniform)
          const float r1 = sqrtf(-2.0f * logf(qs::u01_open0(x.z))), a1 = two_pi * qs::u01_open0(x.w);
          z[2] = r1 * cosf(a1);
          z[3] = r1 * sinf(a1);
        }
      }
      float* out = P.actions + r * (size_t)P.A;
#pragma unroll
      for (int a = 0; a < qs::kPriorMaxAct; ++a) {
        if (a >= P.A) break;
        const float mu = P.action_scale * (s[a] + P.b3[a]);
        const float sg = k != 0 ? P.std_scale * expf(P.logstd[a]) : 0.0f;
        const float val = sg == 0.0f ? mu : mu + sg * z[a];
        out[a] = fminf(fmaxf(val, P.lo), P.hi);
      }
    }
  }
}

struct InjectParams {
  const float* prior;        // [n][per]
  float* cand;               // [n][C · E · D · A]
  uint32_t per;              // K · E · D · A
  size_t step, first;        // C · E · D · A and (C - K) · E · D · A
};

// Step j = blockIdx.y: candidates C - K .. C - 1 become prior_actions[j].
__global__ __launch_bounds__(kValueThreads) void prior_inject_kernel(InjectParams P) {
  const uint32_t t = blockIdx.x * (uint32_t)kValueThreads + threadIdx.x;
  if (t >= P.per) return;
  const size_t j = blockIdx.y;
  P.cand[j * P.step + P.first + t] = P.prior[j * P.per + t];
}

int refuse(const char* who, qs::PriorRefusal r, const qs_prior_spec* s, const qs::PriorShape& shape) {
  const std::string w = std::string(who) + ": ";
  using qs::set_last_error;
  switch (r) {
    case qs::kPriorCount:
      return set_last_error(QS_E_INVALID, w + "count = " + std::to_string(s->count) + " is outside 1 .. candidates - 1 = " +
                                              std::to_string((long long)shape.C - 1) + " (candidate 0 stays the nominal / mean)");
    case qs::kPriorPartNet:
      return set_last_error(QS_E_INVALID, w + "w1, b1, w2, b2, w3, b3 and logstd must all be set");
    case qs::kPriorHidden:
      return set_last_error(QS_E_INVALID, w + "hidden = " + std::to_string(s->hidden) + " is not 64, 128 or 256");
    case qs::kPriorInDim:
      return set_last_error(QS_E_INVALID, w + "in_dim = " + std::to_string(s->in_dim) + " must equal obs_dim = " +
                                              std::to_string((long long)shape.O) + " and be at most " +
                                              std::to_string(qs::kValueMaxIn));
    case qs::kPriorActDim:
      return set_last_error(QS_E_INVALID, w + "act_dim = " + std::to_string(s->act_dim) + " must equal the swarm's act_dim = " +
                                              std::to_string((long long)shape.A) + " and be at most " +
                                              std::to_string(qs::kPriorMaxAct));
    case qs::kPriorPartNorm:
      return set_last_error(QS_E_INVALID, w + "obs_mean and obs_var must be both set or both NULL");
    case qs::kPriorNormArgs:
      return set_last_error(QS_E_INVALID, w + "obs_eps must be finite and >= 0, obs_clip finite and > 0");
    case qs::kPriorNoObs:
      return set_last_error(QS_E_INVALID, w + "obs is NULL (the [num_envs][num_drones][obs_dim] obs of the swarm's current state)");
    case qs::kPriorScales:
      return set_last_error(QS_E_INVALID, w + "std_scale must be finite and >= 0, action_scale finite");
    case qs::kPriorOffsets:
      return set_last_error(QS_E_INVALID, w + "horizon outside 1 .. 32, num_drones above " + std::to_string(qs::kPriorMaxDrones) +
                                              ", or count * num_envs * num_drones * obs_dim * 4 bytes of a step's obs past "
                                              "the 32-bit offsets");
    default:
      return QS_OK;
  }
}

qs::PriorSpecShape spec_shape(const qs_prior_spec* s, int64_t count) {
  qs::PriorSpecShape v;
  v.in_dim = s->in_dim; v.hidden = s->hidden; v.act_dim = s->act_dim; v.count = count;
  v.net_ptrs = (s->w1 != nullptr) + (s->b1 != nullptr) + (s->w2 != nullptr) + (s->b2 != nullptr) + (s->w3 != nullptr) +
               (s->b3 != nullptr) + (s->logstd != nullptr);
  v.mean = s->obs_mean != nullptr;
  v.var = s->obs_var != nullptr;
  v.obs = s->obs != nullptr;
  v.eps = s->obs_eps; v.clip = s->obs_clip; v.action_scale = s->action_scale; v.std_scale = s->std_scale;
  return v;
}

// The actor launch for step j on buffers the caller has checked.
int launch_act(const qs_prior_spec* s, int j, int K, int E, int D, float lo, float hi, uint64_t seed, uint32_t genv0,
               const uint64_t* tick, const float* obs_in, int bcast, float* actions, float* seen, hipStream_t st) {
  PriorParams P;
  P.x = obs_in;
  P.w1 = s->w1; P.b1 = s->b1; P.w2 = s->w2; P.b2 = s->b2; P.w3 = s->w3; P.b3 = s->b3; P.logstd = s->logstd;
  P.mean = s->obs_mean; P.var = s->obs_var;
  P.eps = s->obs_eps; P.clip = s->obs_clip;
  P.actions = actions; P.seen = seen;
  P.tick = tick;
  P.k0 = (uint32_t)seed; P.k1 = (uint32_t)(seed >> 32);
  P.genv0 = genv0; P.j = (uint32_t)j;
  P.ED = (uint32_t)E * (uint32_t)D; P.D = (uint32_t)D;
  P.R = (uint32_t)K * P.ED;
  P.O = s->in_dim; P.A = s->act_dim; P.bcast = bcast ? 1 : 0;
  P.action_scale = s->action_scale; P.std_scale = s->std_scale; P.lo = lo; P.hi = hi;
  const qs::ValuePlan plan = qs::prior_plan(s->hidden, s->in_dim, P.R);
  if (!plan.fits) return qs::set_last_error(QS_E_INVALID, "policy prior: the LDS plan does not fit");
  const dim3 grid(plan.grid), block(kValueThreads);
  const bool wide = plan.tile == 2 * kValueMfmaM;
  if (s->hidden == 64) {
    if (wide) hipLaunchKernelGGL((prior_act_kernel<64, 2>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((prior_act_kernel<64, 1>), grid, block, 0, st, P);
  } else if (s->hidden == 128) {
    if (wide) hipLaunchKernelGGL((prior_act_kernel<128, 2>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((prior_act_kernel<128, 1>), grid, block, 0, st, P);
  } else {
    hipLaunchKernelGGL((prior_act_kernel<256, 1>), grid, block, 0, st, P);
  }
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // namespace

namespace qs {

// What a planner holds once a prior is attached.
struct PriorState {
  qs_prior_spec spec;
  int K, O;
  qs_branch* set;                      // K candidates, forked at every tick
  uint64_t bytes[kPriorBufs];
  void* buf[kPriorBufs];
};

namespace {
float* prior_actions_at(const PlannerBase* p, int j) {
  return (float*)p->prior->buf[kPriorActions] + (size_t)j * ((size_t)p->prior->K * p->E * p->D * p->A);
}
float* prior_obs_at(const PlannerBase* p, int j) {
  return (float*)p->prior->buf[kPriorObs] + (size_t)j * ((size_t)p->prior->K * p->E * p->D * p->prior->O);
}
}  // namespace

void prior_release(PlannerBase* p) {
  if (!p->prior) return;
  qs_branch_destroy(p->prior->set);
  for (void* b : p->prior->buf)
    if (b) (void)hipFree(b);
  delete p->prior;
  p->prior = nullptr;
}

int prior_count(const PlannerBase* p) { return p->prior ? p->prior->K : 0; }

int prior_attach(const char* who, PlannerBase* p, const qs_prior_spec* spec) {
  if (!p) return set_last_error(QS_E_INVALID, std::string(who) + ": null planner");
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (!spec) {   // detach; the work in flight may still read the buffers
    if (p->prior) PLANNER_HIP_TRY(hipDeviceSynchronize());
    prior_release(p);
    return QS_OK;
  }
  qs_dims d;
  if (int rc = qs_get_dims(p->h, &d)) return rc;
  const PriorShape shape{p->n, spec->count, p->C, p->E, p->D, d.obs_dim, p->A};
  if (const PriorRefusal r = prior_refusal(spec_shape(spec, spec->count), shape)) return refuse(who, r, spec, shape);
  if (p->sampling && !sampling_slots_ok(p->C, p->sampling->keep, spec->count))   // (qs_sampling_cem_set: slots 1 .. keep)
    return set_last_error(QS_E_INVALID, std::string(who) + ": 1 + the sampling spec's keep + count = 1 + " +
                                            std::to_string(p->sampling->keep) + " + " + std::to_string(spec->count) +
                                            " is above candidates = " + std::to_string(p->C) +
                                            " (the mean, the kept elites and the prior's rollouts each need their own slots)");
  PriorState* v = new (std::nothrow) PriorState;
  if (!v) return set_last_error(QS_E_NOMEM, std::string(who) + ": out of host memory");
  v->spec = *spec;
  v->K = spec->count;
  v->O = d.obs_dim;
  v->set = nullptr;
  (void)prior_sizes(shape, v->bytes);   // (prior_refusal has accepted it)
  for (void*& b : v->buf) b = nullptr;
  if (int rc = qs_branch_create(p->h, v->K, &v->set)) {   // (its own refusals and message)
    delete v;
    return rc;
  }
  hipError_t e = hipSuccess;
  for (int i = 0; i < kPriorBufs && e == hipSuccess; ++i) {
    e = hipMalloc(&v->buf[i], v->bytes[i]);
    if (e == hipSuccess) e = hipMemset(v->buf[i], 0, v->bytes[i]);
  }
  if (e != hipSuccess) {
    for (void* b : v->buf)
      if (b) (void)hipFree(b);
    qs_branch_destroy(v->set);
    delete v;
    return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  if (p->prior) {   // replaced; the work in flight may still read the old buffers
    (void)hipDeviceSynchronize();
    prior_release(p);
  }
  p->prior = v;
  return QS_OK;
}

int prior_buffers(const char* who, const PlannerBase* p, float** prior_actions, float** prior_obs) {
  if (!p || !prior_actions || !prior_obs) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  const PriorState* v = p->prior;
  *prior_actions = v ? (float*)v->buf[kPriorActions] : nullptr;
  *prior_obs = v ? (float*)v->buf[kPriorObs] : nullptr;
  return QS_OK;
}

int prior_rollout(const char* who, PlannerBase* p, uint64_t seed, const uint64_t* tick, float lo, float hi, void* stream) {
  PriorState* v = p->prior;
  if (!v) return set_last_error(QS_E_STATE, std::string(who) + ": no prior is attached");
  if (int rc = qs_branch_fork(v->set, stream)) return rc;
  for (int j = 0; j < p->n; ++j) {
    float* act = prior_actions_at(p, j);
    if (int rc = launch_act(&v->spec, j, v->K, p->E, p->D, lo, hi, seed, (uint32_t)p->info.env_offset, tick,
                            j == 0 ? v->spec.obs : prior_obs_at(p, j), j == 0, act, j == 0 ? prior_obs_at(p, 0) : nullptr,
                            (hipStream_t)stream))
      return rc;
    if (j == p->n - 1) break;
    const float* step = act;
    qs_step_out out{};
    out.obs = prior_obs_at(p, j + 1);
    if (int rc = qs_branch_advance(v->set, 1, &step, &out, stream)) return rc;
  }
  return QS_OK;
}

int prior_inject(PlannerBase* p, float* candidates, void* stream) {
  const PriorState* v = p->prior;
  if (!v) return QS_OK;
  InjectParams P;
  const size_t row = (size_t)p->E * p->D * p->A;
  P.prior = (const float*)v->buf[kPriorActions];
  P.cand = candidates;
  P.per = (uint32_t)((size_t)v->K * row);
  P.step = (size_t)p->C * row;
  P.first = (size_t)(p->C - v->K) * row;
  hipLaunchKernelGGL(prior_inject_kernel, dim3(prior_inject_grid(v->K, p->E, p->D, p->A), (uint32_t)p->n), dim3(kValueThreads),
                     0, (hipStream_t)stream, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // namespace qs

extern "C" {

int qs_prior_act(const qs_prior_spec* spec, int j, int K, int E, int D, float lo, float hi, uint64_t seed, int64_t genv0,
                 const uint64_t* tick, const float* obs_in, int bcast, float* actions_out, float* obs_seen, void* stream) {
  const char* who = "qs_prior_act";
  using qs::set_last_error;
  if (!spec || !tick || !obs_in || !actions_out) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  if (j < 0 || j >= qs::kValueMaxSteps || K < 1 || E < 1 || D < 1)
    return set_last_error(QS_E_INVALID, std::string(who) + ": j must be in 0 .. 31, K, E and D >= 1");
  if (!(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi))
    return set_last_error(QS_E_INVALID, std::string(who) + ": lo must be below hi, both finite");
  if (obs_seen == obs_in) return set_last_error(QS_E_INVALID, std::string(who) + ": obs_seen is obs_in (pass NULL for no copy)");
  qs_prior_spec s = *spec;
  s.obs = obs_in;
  const qs::PriorShape shape{1, K, (int64_t)K + 1, E, D, s.in_dim, s.act_dim};
  if (const qs::PriorRefusal r = qs::prior_refusal(spec_shape(&s, K), shape)) return refuse(who, r, &s, shape);
  return launch_act(&s, j, K, E, D, lo, hi, seed, (uint32_t)genv0, tick, obs_in, bcast, actions_out, obs_seen,
                    (hipStream_t)stream);
}

}  // extern "C"
