// planner_value.hip — the value tail of a branch rollout (include/quadswarm.h,
// qs_value_tail, qs_value_mppi_set / qs_value_cem_set; DESIGN.md §4a "Value tail").
//
// One launch over the V = C · E virtual envs of a qs_score call: gather the row of
// D · O floats the rollout wrote as its last obs, normalise it (float64, the
// expression of qs_rms_normalize), run the critic's tanh MLP on the f32-input MFMA
// with the activations kept in LDS between the layers, write value[c][e], and
// fold the discounted rewards and the bootstrap term into ret[c][e] in float64.
// The weights are read from the caller's nn.Linear tensors at every launch (no
// pack step), W1 and W2 streamed through LDS in K-chunks.  No atomics and a fixed
// summation order: the same inputs give the same bytes.  The host arithmetic
// (refusals, sizes, tile, grid, LDS plan, discount table) is value_sizes.h.
#include "planner_common.h"
#include "value_sizes.h"

namespace {

using qs::kValueChunk;
using qs::kValueMfmaK;
using qs::kValueMfmaM;
using qs::kValuePad;
using qs::kValueThreads;
using qs::kValueWaves;

typedef float value_f4 __attribute__((ext_vector_type(4)));

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

// out = clip((x − mean) / sqrt(var + eps), ±clip) in float64, rounded to float32:
// rms_norm1 of normalizer.hip.
__device__ __forceinline__ float norm1(float xv, double m, double sd, double clip) {
  double y = ((double)xv - m) / sd;
  y = y < -clip ? -clip : (y > clip ? clip : y);
  return (float)y;
}

// One layer's product for a workgroup's rows: acc[mt][nt] += A · Wᵀ over K, with W
// [N][K] row-major in global memory streamed through sW in chunks of kValueChunk
// columns (zero beyond K).  FIRST: A is the input, staged (and normalised) a chunk
// at a time into sX; otherwise A is sH, resident.  Wave w owns the column tiles
// w · NT .. w · NT + NT - 1 of all MT row tiles.  The next chunk's global loads are
// issued before the current chunk's MFMAs and land in LDS after them.
template <int N, int MT, bool FIRST>
__device__ __forceinline__ void layer_product(const ValueParams& P, const float* __restrict__ W, int K, size_t row0,
                                              float* sH, float* sW, float* sX, value_f4 (&acc)[MT][N / 64]) {
  constexpr int NT = N / 64, TM = MT * kValueMfmaM, CP = kValueChunk + kValuePad, HP = N + kValuePad;
  constexpr int WR = N / 8, XR = TM / 8;   // rows of W / X a thread stages per chunk (32 columns x 8 rows a pass)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, rsub = tid >> 5;   // this thread's column of a chunk, and its first row
  const int l15 = lane & 15, lq = lane >> 4;
  float wreg[WR], xreg[FIRST ? XR : 1];
  const int chunks = (K + kValueChunk - 1) / kValueChunk;

  auto load = [&](int ch) {
    const int k = ch * kValueChunk + col;
    const bool kv = k < K;
#pragma unroll
    for (int i = 0; i < WR; ++i) wreg[i] = kv ? W[(size_t)(rsub + 8 * i) * K + k] : 0.0f;
    if constexpr (FIRST) {
      double m = 0.0, sd = 1.0;
      if (P.mean && kv) {
        m = P.mean[k];
        sd = sqrt(P.var[k] + P.eps);
      }
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        const size_t r = row0 + (size_t)(rsub + 8 * i);
        float xv = 0.0f;
        if (kv && r < (size_t)P.V) {
          xv = P.x[r * (size_t)K + k];
          if (P.mean) xv = norm1(xv, m, sd, P.clip);
        }
        xreg[i] = xv;
      }
    }
  };

  load(0);
  for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll
    for (int i = 0; i < WR; ++i) sW[(rsub + 8 * i) * CP + col] = wreg[i];
    if constexpr (FIRST) {
#pragma unroll
      for (int i = 0; i < XR; ++i) sX[(rsub + 8 * i) * CP + col] = xreg[i];
    }
    __syncthreads();
    if (ch + 1 < chunks) load(ch + 1);
    const int left = K - ch * kValueChunk;
    const int ksteps = left >= kValueChunk ? kValueChunk / kValueMfmaK : (left + kValueMfmaK - 1) / kValueMfmaK;
    const float* A = FIRST ? sX : sH + ch * kValueChunk;
    constexpr int AP = FIRST ? CP : HP;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int kk = ks * kValueMfmaK + lq;
      float a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = A[(mt * kValueMfmaM + l15) * AP + kk];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = sW[((wave * NT + nt) * kValueMfmaM + l15) * CP + kk];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    __syncthreads();   // sW / sX are rewritten by the next trip (and sH by the caller)
  }
}

// The accumulators' (row, column) of register r: row = 4 · (lane >> 4) + r, column = lane & 15.
template <int N, int MT>
__global__ __launch_bounds__(kValueThreads) void value_mlp_kernel(ValueParams P) {
  constexpr int NT = N / 64, TM = MT * kValueMfmaM, CP = kValueChunk + kValuePad, HP = N + kValuePad;
  __shared__ float sH[TM * HP];
  __shared__ float sW[N * CP];
  __shared__ float sX[TM * CP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * TM;
  value_f4 acc[MT][NT];
  auto clear = [&]() {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = value_f4{0.0f, 0.0f, 0.0f, 0.0f};
  };

  // H1 = tanh(X · W1ᵀ + b1) into sH
  clear();
  layer_product<N, MT, true>(P, P.w1, P.I, row0, sH, sW, sX, acc);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int nc = (wave * NT + nt) * kValueMfmaM + l15;
    const float bias = P.b1[nc];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sH[(mt * kValueMfmaM + 4 * lq + r) * HP + nc] = tanhf(acc[mt][nt][r] + bias);
  }
  __syncthreads();

  // H2 = tanh(H1 · W2ᵀ + b2); sH becomes H2 · w3, column by column
  clear();
  layer_product<N, MT, false>(P, P.w2, N, row0, sH, sW, sX, acc);   // (ends in a barrier: every wave is done with H1)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int nc = (wave * NT + nt) * kValueMfmaM + l15;
    const float bias = P.b2[nc], w3 = P.w3[nc];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sH[(mt * kValueMfmaM + 4 * lq + r) * HP + nc] = tanhf(acc[mt][nt][r] + bias) * w3;
  }
  __syncthreads();

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
