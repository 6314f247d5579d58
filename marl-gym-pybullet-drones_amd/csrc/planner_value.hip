// planner_value.hip — the value tail of a branch rollout (include/quadswarm.h,
// qs_value_tail, qs_value_mppi_set / qs_value_cem_set; DESIGN.md §4a "Value tail").
//
// One launch over the V = C · E virtual envs of a qs_score call: gather the row of
// D · O floats the rollout wrote as its last obs, normalise it (float64, the
// expression of qs_rms_normalize), run the critic's tanh MLP on the f32-input MFMA
// with the activations kept in LDS between the layers, write value[c][e], and
// fold the discounted rewards and the bootstrap term into ret[c][e] in float64.
// The weights are read from the caller's nn.Linear tensors at every launch (no
// pack step), W1 and W2 streamed through LDS in K-chunks (mlp_tile.h, shared with
// the policy prior).  No atomics and a fixed
// summation order: the same inputs give the same bytes.  The host arithmetic
// (refusals, sizes, tile, grid, LDS plan, discount table) is value_sizes.h.
#include "planner_common.h"
#include "mlp_tile.h"

namespace {

using qs::kValueChunk;
using qs::kValueMfmaM;
using qs::kValuePad;
using qs::kValueThreads;

struct FoldParams {
  double* ret;                               // [V], rewritten in place
  const int32_t* first_done;                 // [V]
  const void* rewards[qs::kValueMaxSteps];   // step j's [V] reals; read only where discounts != 0
  double disc[qs::kValueMaxSteps + 1];
  double boot;                               // disc[n] · scale
  int n, real_bytes, discounts;
};

struct ValueParams {
  const float* x;                            // last_obs [V][I]
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  const double *mean, *var;                  // [I], or both null
  double eps, clip;
  float* value;                              // [V]
  int V, I;
  FoldParams F;
};

// §1.5 of the contract, for row v.  has_value: a net ran and `val` is its output.
__device__ __forceinline__ void fold_row(const FoldParams& F, size_t v, bool has_value, float val) {
  const int jd = F.first_done[v];
  double acc;
  if (F.discounts) {
    acc = 0.0;
    const int last = jd < F.n - 1 ? jd : F.n - 1;
    for (int j = 0; j <= last; ++j) {
      const double r = F.real_bytes == 8 ? ((const double*)F.rewards[j])[v] : (double)((const float*)F.rewards[j])[v];
      acc = acc + F.disc[j] * r;
    }
  } else {
    acc = F.ret[v];
  }
  if (has_value && jd == F.n) acc = acc + F.boot * (double)val;
  F.ret[v] = acc;
}

__global__ __launch_bounds__(kValueThreads) void value_fold_kernel(FoldParams F, int V) {
  const uint32_t v = blockIdx.x * (uint32_t)kValueThreads + threadIdx.x;
  if (v < (uint32_t)V) fold_row(F, v, false, 0.0f);
}

// The rows of last_obs as the critic takes them (mlp_tile.h, layer_product's
// input): column k normalised by entry k of the statistics.
struct ValueInput {
  const float* x;                            // [rows][I]
  const double *mean, *var;
  double eps, clip;
  size_t rows;
  int I;
  template <int XR>
  __device__ __forceinline__ void stage(size_t r0, int k, bool kv, float (&out)[XR]) const {
    double m = 0.0, sd = 1.0;
    if (mean && kv) {
      m = mean[k];
      sd = sqrt(var[k] + eps);
    }
#pragma unroll
    for (int i = 0; i < XR; ++i) {
      const size_t r = r0 + (size_t)(8 * i);
      float xv = 0.0f;
      if (kv && r < rows) {
        xv = x[r * (size_t)I + k];
        if (mean) xv = qs::norm1(xv, m, sd, clip);
      }
      out[i] = xv;
    }
  }
};

template <int N, int MT>
__global__ __launch_bounds__(kValueThreads) void value_mlp_kernel(ValueParams P) {
  constexpr int TM = MT * kValueMfmaM, CP = kValueChunk + kValuePad, HP = N + kValuePad;
  __shared__ float sH[TM * HP];
  __shared__ float sW[N * CP];
  __shared__ float sX[TM * CP];
  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * TM;
  // sH = tanh(tanh(X · W1ᵀ + b1) · W2ᵀ + b2) · w3, column by column
  const ValueInput in{P.x, P.mean, P.var, P.eps, P.clip, (size_t)P.V, P.I};
  qs::hidden_layers<N, MT>(in, P.I, P.w1, P.b1, P.w2, P.b2, P.w3, row0, sH, sW, sX);

  // V = Σ_n sH[row][n] + b3: eight lanes a row, each over n = part, part + 8, ..., then an xor tree
  if (tid < TM * 8) {   // (whole waves: TM · 8 is 128 or 256)
    const int row = tid >> 3, part = tid & 7;
    float s = 0.0f;
    for (int nn = part; nn < N; nn += 8) s += sH[row * HP + nn];
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    const size_t v = row0 + (size_t)row;
    if (part == 0 && v < (size_t)P.V) {
      const float val = s + P.b3[0];
      P.value[v] = val;
      fold_row(P.F, v, true, val);
    }
  }
}

int refuse(const char* who, qs::ValueRefusal r, const qs_value_spec* s, int D, int O) {
  const std::string w = std::string(who) + ": ";
  using qs::set_last_error;
  switch (r) {
    case qs::kValuePerDrone:
      return set_last_error(QS_E_INVALID, w + "this is a per-drone planner: a centralized critic has one value per env, "
                                              "not one per drone (attach it to an env-level planner)");
    case qs::kValueInDim:
      return set_last_error(QS_E_INVALID, w + "in_dim = " + std::to_string(s->in_dim) + " must equal num_drones * obs_dim = " +
                                              std::to_string((long long)D * O) + " and be at most " +
                                              std::to_string(qs::kValueMaxIn));
    case qs::kValueHidden:
      return set_last_error(QS_E_INVALID, w + "hidden = " + std::to_string(s->hidden) + " is not 64, 128 or 256");
    case qs::kValuePartNet:
      return set_last_error(QS_E_INVALID, w + "w1, b1, w2, b2, w3 and b3 must be all set (a net) or all NULL (discount only)");
    case qs::kValuePartNorm:
      return set_last_error(QS_E_INVALID, w + "obs_mean and obs_var must be both set or both NULL");
    case qs::kValueNormNoNet:
      return set_last_error(QS_E_INVALID, w + "obs_mean / obs_var without a net");
    case qs::kValueNormArgs:
      return set_last_error(QS_E_INVALID, w + "obs_eps must be finite and >= 0, obs_clip finite and > 0");
    case qs::kValueGamma:
      return set_last_error(QS_E_INVALID, w + "gamma must be in (0, 1]");
    case qs::kValueScale:
      return set_last_error(QS_E_INVALID, w + "scale must be finite");
    case qs::kValueOffsets:
      return set_last_error(QS_E_INVALID, w + "horizon outside 1 .. 32, or candidates * num_envs * num_drones * obs_dim * 4 "
                                              "bytes of last_obs (or a step of rewards) past the 32-bit offsets");
    default:
      return QS_OK;
  }
}

qs::ValueSpecShape spec_shape(const qs_value_spec* s) {
  qs::ValueSpecShape v;
  v.in_dim = s->in_dim;
  v.hidden = s->hidden;
  v.net_ptrs = (s->w1 != nullptr) + (s->b1 != nullptr) + (s->w2 != nullptr) + (s->b2 != nullptr) + (s->w3 != nullptr) +
               (s->b3 != nullptr);
  v.mean = s->obs_mean != nullptr;
  v.var = s->obs_var != nullptr;
  v.eps = s->obs_eps; v.clip = s->obs_clip; v.gamma = s->gamma; v.scale = s->scale;
  return v;
}

// The launch (or none: no net and gamma = 1) on buffers the caller has checked.
int launch_tail(const qs_value_spec* s, int n, int64_t V, int real_bytes, const float* last_obs,
                const void* const* rewards, double* ret, const int32_t* first_done, float* value, hipStream_t st) {
  const bool net = s->w1 != nullptr, discounts = qs::value_discounts(s->gamma);
  if (!net && !discounts) return QS_OK;
  ValueParams P;
  FoldParams& F = P.F;
  F.ret = ret;
  F.first_done = first_done;
  for (int j = 0; j < qs::kValueMaxSteps; ++j) F.rewards[j] = discounts && j < n ? rewards[j] : nullptr;
  for (double& d : F.disc) d = 0.0;
  qs::value_disc(s->gamma, n, F.disc);
  F.boot = F.disc[n] * s->scale;
  F.n = n; F.real_bytes = real_bytes; F.discounts = discounts ? 1 : 0;
  if (!net) {
    hipLaunchKernelGGL(value_fold_kernel, dim3(qs::value_fold_grid(V)), dim3(kValueThreads), 0, st, F, (int)V);
    PLANNER_HIP_TRY(hipGetLastError());
    return QS_OK;
  }
  P.x = last_obs;
  P.w1 = s->w1; P.b1 = s->b1; P.w2 = s->w2; P.b2 = s->b2; P.w3 = s->w3; P.b3 = s->b3;
  P.mean = s->obs_mean; P.var = s->obs_var;
  P.eps = s->obs_eps; P.clip = s->obs_clip;
  P.value = value;
  P.V = (int)V; P.I = s->in_dim;
  const qs::ValuePlan plan = qs::value_plan(s->hidden, s->in_dim, V);
  if (!plan.fits) return qs::set_last_error(QS_E_INVALID, "value tail: the LDS plan does not fit");
  const dim3 grid(plan.grid), block(kValueThreads);
  const bool wide = plan.tile == 2 * kValueMfmaM;
  if (s->hidden == 64) {
    if (wide) hipLaunchKernelGGL((value_mlp_kernel<64, 2>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((value_mlp_kernel<64, 1>), grid, block, 0, st, P);
  } else if (s->hidden == 128) {
    if (wide) hipLaunchKernelGGL((value_mlp_kernel<128, 2>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((value_mlp_kernel<128, 1>), grid, block, 0, st, P);
  } else {
    hipLaunchKernelGGL((value_mlp_kernel<256, 1>), grid, block, 0, st, P);
  }
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // namespace

namespace qs {

// What a planner holds once a value is attached.
struct ValueState {
  qs_value_spec spec;
  int real_bytes;
  uint64_t bytes[kValueBufs];
  void* buf[kValueBufs];
  std::vector<qs_step_out> outs;       // the n step outputs the score launch names
  std::vector<const void*> rewards;    // step j's rewards, or empty
};

void value_release(PlannerBase* p) {
  if (!p->value) return;
  for (void* b : p->value->buf)
    if (b) (void)hipFree(b);
  delete p->value;
  p->value = nullptr;
}

int value_attach(const char* who, PlannerBase* p, const qs_value_spec* spec) {
  if (!p) return set_last_error(QS_E_INVALID, std::string(who) + ": null planner");
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (!spec) {   // detach; the work in flight may still read the buffers
    if (p->value) PLANNER_HIP_TRY(hipDeviceSynchronize());
    value_release(p);
    return QS_OK;
  }
  if (track_attached(p))
    return set_last_error(QS_E_INVALID, std::string(who) + ": a tracking spec is attached: the tail's discounted return and "
                                                           "the undiscounted tracking cost do not compose (detach it first)");
  if (avoid_attached(p))
    return set_last_error(QS_E_INVALID, std::string(who) + ": an avoidance spec is attached: the tail's discounted return and "
                                                           "the undiscounted avoidance cost do not compose (detach it first)");
  qs_dims d;
  if (int rc = qs_get_dims(p->h, &d)) return rc;
  const ValueShape shape{p->n, p->C, p->E, p->D, d.obs_dim, d.precision};
  if (const ValueRefusal r = value_refusal(spec_shape(spec), shape, p->per_drone)) return refuse(who, r, spec, p->D, d.obs_dim);
  ValueState* v = new (std::nothrow) ValueState;
  if (!v) return set_last_error(QS_E_NOMEM, std::string(who) + ": out of host memory");
  v->spec = *spec;
  v->real_bytes = d.precision;
  const bool net = spec->w1 != nullptr, discounts = value_discounts(spec->gamma);
  (void)value_sizes(shape, net, discounts, v->bytes);   // (value_refusal has accepted it)
  for (void*& b : v->buf) b = nullptr;
  hipError_t e = hipSuccess;
  for (int i = 0; i < kValueBufs && e == hipSuccess; ++i) {
    if (v->bytes[i] == 0) continue;
    e = hipMalloc(&v->buf[i], v->bytes[i]);
    if (e == hipSuccess) e = hipMemset(v->buf[i], 0, v->bytes[i]);
  }
  if (e != hipSuccess) {
    for (void* b : v->buf)
      if (b) (void)hipFree(b);
    delete v;
    return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  if (net || discounts) {
    v->outs.assign((size_t)p->n, qs_step_out{});
    if (net) v->outs[(size_t)p->n - 1].obs = (float*)v->buf[kValueLastObs];
    if (discounts) {
      const size_t step = (size_t)(v->bytes[kValueRewards] / (uint64_t)p->n);
      for (int j = 0; j < p->n; ++j) {
        v->outs[(size_t)j].reward = (char*)v->buf[kValueRewards] + (size_t)j * step;
        v->rewards.push_back(v->outs[(size_t)j].reward);
      }
    }
  }
  if (p->value) {   // replaced; the work in flight may still read the old buffers
    (void)hipDeviceSynchronize();
    value_release(p);
  }
  p->value = v;
  return QS_OK;
}

int value_buffers(const char* who, const PlannerBase* p, float** last_obs, float** value, void** rewards) {
  if (!p || !last_obs || !value || !rewards) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  const ValueState* v = p->value;
  *last_obs = v ? (float*)v->buf[kValueLastObs] : nullptr;
  *value = v ? (float*)v->buf[kValueOut] : nullptr;
  *rewards = v ? v->buf[kValueRewards] : nullptr;
  return QS_OK;
}

int value_score(PlannerBase* p, void* ret, void* first_done, void* stream) {
  ValueState* v = p->value;
  if (!v || v->outs.empty()) return planner_score(p, ret, first_done, stream);   // (no value, or no net and gamma = 1)
  const qs_score_out so{ret, (int32_t*)first_done};
  if (int rc = qs_score(p->h, p->n, p->C, p->steps.data(), v->outs.data(), &so, stream)) return rc;
  return launch_tail(&v->spec, p->n, (int64_t)p->C * p->E, v->real_bytes, (const float*)v->buf[kValueLastObs],
                     v->rewards.empty() ? nullptr : v->rewards.data(), (double*)ret, (const int32_t*)first_done,
                     (float*)v->buf[kValueOut], (hipStream_t)stream);
}

}  // namespace qs

extern "C" {

int qs_value_tail(const qs_value_spec* spec, int n, int C, int E, int D, int O, int real_bytes, const float* last_obs,
                  const void* const* rewards, double* ret, const int32_t* first_done, float* value_out, void* stream) {
  const char* who = "qs_value_tail";
  using qs::set_last_error;
  if (!spec || !ret || !first_done) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  const qs::ValueShape shape{n, C, E, D, O, real_bytes};
  if (n < 1 || n > qs::kValueMaxSteps || C < 1 || E < 1 || D < 1 || O < 1 || (real_bytes != 4 && real_bytes != 8))
    return set_last_error(QS_E_INVALID, std::string(who) + ": n must be in 1 .. 32, C, E, D and O >= 1, real_bytes 4 or 8");
  if (const qs::ValueRefusal r = qs::value_refusal(spec_shape(spec), shape, false)) return refuse(who, r, spec, D, O);
  const bool net = spec->w1 != nullptr, discounts = qs::value_discounts(spec->gamma);
  if (net && (!last_obs || !value_out))
    return set_last_error(QS_E_INVALID, std::string(who) + ": a net needs last_obs and value_out");
  if (discounts) {
    if (!rewards) return set_last_error(QS_E_INVALID, std::string(who) + ": gamma != 1 needs the n steps' rewards");
    for (int j = 0; j < n; ++j)
      if (!rewards[j]) return set_last_error(QS_E_INVALID, std::string(who) + ": a NULL among rewards[]");
  }
  return launch_tail(spec, n, (int64_t)C * E, real_bytes, last_obs, rewards, ret, first_done, value_out, (hipStream_t)stream);
}

}  // extern "C"
