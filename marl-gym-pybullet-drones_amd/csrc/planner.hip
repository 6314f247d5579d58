// planner.hip — the MPPI planner tick on top of qs_score (include/quadswarm.h,
// qs_mppi_*; DESIGN.md §4a "Planner tick").
//
// Three kernels round the one qs_score launch: planner_sample_kernel (shared with
// the CEM tick, planner_common.h) perturbs the nominal sequence into C candidates
// (with a policy prior attached, planner_prior.hip, the last of them are then
// overwritten with the actor's closed-loop rollouts; with a sampling spec that has a
// non-zero rho, qs_sampling_mppi_set, planner_sample_ar_kernel takes its place: the
// same launch count, time-correlated noise),
// mppi_weights_* turns qs_score's ret / first_done into softmax weights per env,
// and mppi_sum_* folds the candidates back into the nominal, shifted by one step.
// Everything per env is summed in double in a fixed order (no atomics), the tick
// counter lives on the device, and nothing is read back, so a tick can be captured
// and replayed.  The host arithmetic (sizes, variant, grids) is planner_sizes.h.
#include "planner_common.h"

namespace {

// The spread of component a, from the kernel arguments.
struct SigmaArg {
  float sigma[4];
  __device__ __forceinline__ float at(size_t, int a) const { return sigma[a]; }
};

struct UpdateParams {
  // E counts the units that are weighed on their own and row their components:
  // the envs and D · A, or in per-drone mode the E · D agents and A
  // (planner_common.h, PlannerBase).  Either way [E][row] is [envs][D][A].
  const float* cand;         // [n][C][E][row]
  const double* ret;         // [C][E]: ret, or in per-drone mode ret_agent
  const int32_t* first_done; // [C][E / fd_div]
  double* w;                 // [C][E]
  int32_t* best;             // [E]
  float* nominal;            // [n][E][row]
  float* action;             // [E][row]
  uint64_t* tick;
  double lambda, penalty;
  int n, C, E, row, rowp;    // rowp = the power of two >= row
  int fd_div;                // 1, or in per-drone mode D
};

using qs::score_of;
// The better of two (score, candidate) pairs: the larger score, the lower c on a tie.
__device__ __forceinline__ void take_better(double& s, int& c, double s2, int c2) {
  if (s2 > s || (s2 == s && c2 < c)) { s = s2; c = c2; }
}

// ---- weights, one thread per env ------------------------------------------
__global__ __launch_bounds__(qs::kMppiThreads) void mppi_weights_thread_kernel(UpdateParams P) {
  const int e = blockIdx.x * qs::kMppiThreads + threadIdx.x;
  if (e >= P.E) return;
  double sb = score_of(P, e);
  int cb = 0;
  for (int c = 1; c < P.C; ++c) take_better(sb, cb, score_of(P, (size_t)c * P.E + e), c);
  P.best[e] = cb;
  if (P.lambda == 0.0) {
    for (int c = 0; c < P.C; ++c) P.w[(size_t)c * P.E + e] = c == cb ? 1.0 : 0.0;
    return;
  }
  double sum = 0.0;
  for (int c = 0; c < P.C; ++c) {
    const size_t ce = (size_t)c * P.E + e;
    const double x = exp((score_of(P, ce) - sb) / P.lambda);
    P.w[ce] = x;
    sum += x;
  }
  for (int c = 0; c < P.C; ++c) P.w[(size_t)c * P.E + e] /= sum;
}

// ---- weights, one workgroup per env -----------------------------------------
// Each thread strides over c; the arg max and the sum of exponentials go through
// an in-wave xor tree and then the sixteen waves' partials in LDS, in a fixed order.
__global__ __launch_bounds__(qs::kMppiSumThreads) void mppi_weights_block_kernel(UpdateParams P) {
  constexpr int kThreads = qs::kMppiSumThreads, kWaves = kThreads / 64;
  __shared__ double sh_s[kWaves];
  __shared__ int sh_c[kWaves];
  __shared__ double sh_sum[kWaves];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double sb = -INFINITY;
  int cb = INT32_MAX;
  for (int c = tid; c < P.C; c += kThreads) take_better(sb, cb, score_of(P, (size_t)c * P.E + e), c);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double s2 = __shfl_xor(sb, off, 64);
    const int c2 = __shfl_xor(cb, off, 64);
    take_better(sb, cb, s2, c2);
  }
  if (lane == 0) { sh_s[wave] = sb; sh_c[wave] = cb; }
  __syncthreads();
  sb = sh_s[0];
  cb = sh_c[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) take_better(sb, cb, sh_s[k], sh_c[k]);
  if (cb >= P.C) cb = 0;   // every score a NaN: no comparison held; best stays an index the sum may read
  if (tid == 0) P.best[e] = cb;
  if (P.lambda == 0.0) {
    for (int c = tid; c < P.C; c += kThreads) P.w[(size_t)c * P.E + e] = c == cb ? 1.0 : 0.0;
    return;
  }
  double sum = 0.0;
  for (int c = tid; c < P.C; c += kThreads) {
    const size_t ce = (size_t)c * P.E + e;
    const double x = exp((score_of(P, ce) - sb) / P.lambda);
    P.w[ce] = x;   // (this thread reads it back below)
    sum += x;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) sh_sum[wave] = sum;
  __syncthreads();
  double part[kWaves];   // every thread folds the same partials in the same pairwise order
#pragma unroll
  for (int k = 0; k < kWaves; ++k) part[k] = sh_sum[k];
#pragma unroll
  for (int w = 1; w < kWaves; w <<= 1) {
#pragma unroll
    for (int k = 0; k < kWaves; k += 2 * w) part[k] += part[k + w];
  }
  sum = part[0];
  for (int c = tid; c < P.C; c += kThreads) P.w[(size_t)c * P.E + e] /= sum;
}

// new[j][e][k] goes where the shifted nominal wants it.  Nothing here reads the
// nominal (candidate 0 holds its copy), so the shift has nothing to overtake.
__device__ __forceinline__ void store_new(const UpdateParams& P, int j, int e, int k, float v) {
  const size_t ek = (size_t)e * P.row + k, step = (size_t)P.E * P.row;
  if (j == 0) P.action[ek] = v;
  else P.nominal[(size_t)(j - 1) * step + ek] = v;
  if (j == P.n - 1) P.nominal[(size_t)j * step + ek] = v;   // hold
}

// ---- weighted sum, one thread per (j, e, d, a) --------------------------------
__global__ __launch_bounds__(qs::kMppiThreads) void mppi_sum_thread_kernel(UpdateParams P) {
  const uint64_t t = (uint64_t)blockIdx.x * qs::kMppiThreads + threadIdx.x;
  if (t == 0) *P.tick += 1;
  const size_t step = (size_t)P.E * P.row;
  if (t >= (uint64_t)P.n * step) return;
  const int j = (int)(t / step);
  const size_t ek = t % step;
  const int e = (int)(ek / P.row), k = (int)(ek % P.row);
  const float* cj = P.cand + (size_t)j * P.C * step + ek;
  float v;
  if (P.lambda == 0.0) {
    v = cj[(size_t)P.best[e] * step];
  } else {
    double acc = 0.0;
    for (int c = 0; c < P.C; ++c) acc += P.w[(size_t)c * P.E + e] * (double)cj[(size_t)c * step];
    v = (float)acc;
  }
  store_new(P, j, e, k, v);
}

// ---- weighted sum, one workgroup per (env, step) ------------------------------
// Thread t holds component k = t mod rowp of candidate group g = t / rowp and
// strides over c by the group count; block_row_reduce sums the groups.
__global__ __launch_bounds__(qs::kMppiSumThreads) void mppi_sum_block_kernel(UpdateParams P) {
  __shared__ double part[qs::kMppiSumThreads];   // [partials][rowp], at most 16 · 64 or 1024 / rowp · rowp
  const int e = blockIdx.x % P.E, j = blockIdx.x / P.E;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) *P.tick += 1;
  const int rowp = P.rowp, k = tid & (rowp - 1), g = tid / rowp, G = qs::kMppiSumThreads / rowp;
  const size_t step = (size_t)P.E * P.row;
  const float* cj = P.cand + (size_t)j * P.C * step + (size_t)e * P.row;
  if (P.lambda == 0.0) {
    if (tid < P.row) store_new(P, j, e, tid, cj[(size_t)P.best[e] * step + tid]);
    return;
  }
  double acc = 0.0;
  if (k < P.row) {
#pragma unroll 4
    for (int c = g; c < P.C; c += G) acc += P.w[(size_t)c * P.E + e] * (double)cj[(size_t)c * step + k];
  }
  qs::block_row_reduce(acc, part, tid, rowp);
  if (tid < P.row) store_new(P, j, e, tid, (float)part[tid]);
}

}  // namespace

struct qs_mppi : qs::PlannerBase {
  qs_mppi_spec spec;
  qs::MppiVariant variant;
  qs::MppiGrids grids;
  uint64_t bytes[qs::kMppiBufs];
  void* buf[qs::kMppiBufs];
};

namespace {

UpdateParams update_params(const qs_mppi* p) {
  UpdateParams P;
  P.cand = (const float*)p->buf[qs::kMppiCandidates];
  P.ret = p->scores(p->buf[qs::kMppiRet]);
  P.first_done = (const int32_t*)p->buf[qs::kMppiFirstDone];
  P.w = (double*)p->buf[qs::kMppiWeights];
  P.best = (int32_t*)p->buf[qs::kMppiBest];
  P.nominal = (float*)p->buf[qs::kMppiNominal];
  P.action = (float*)p->buf[qs::kMppiAction];
  P.tick = (uint64_t*)p->buf[qs::kMppiTick];
  P.lambda = p->spec.lambda;
  P.penalty = p->spec.done_penalty;
  P.n = p->n; P.C = p->C; P.E = p->units();
  P.row = p->row();
  P.rowp = qs::mppi_row_pow2(P.row);
  P.fd_div = p->fd_div();
  return P;
}

// The shared sample kernel round the nominal, its spread from the arguments: tag 3, no iteration.
int sample_impl(qs_mppi* p, hipStream_t st) {
  qs::SampleParams<SigmaArg> P;
  P.mean = (const float*)p->buf[qs::kMppiNominal];
  P.cand = (float*)p->buf[qs::kMppiCandidates];
  P.tick = (const uint64_t*)p->buf[qs::kMppiTick];
  P.k0 = (uint32_t)p->spec.seed; P.k1 = (uint32_t)(p->spec.seed >> 32);
  P.genv0 = (uint32_t)p->info.env_offset;
  P.tag = (uint32_t)qs::kMppiTag; P.iter = 0;
  P.n = p->n; P.C = p->C; P.E = p->E; P.D = p->D; P.A = p->A;
  for (int a = 0; a < 4; ++a) P.spread.sigma[a] = p->spec.sigma[a];
  P.lo = p->spec.lo; P.hi = p->spec.hi;
  if (int rc = qs::planner_launch_sample(p, P, p->grids.sample, st)) return rc;   // (serial in j with a correlated sampling spec)
  return qs::prior_inject(p, P.cand, st);   // (nothing without a prior)
}

// The prior stage, keyed as the sample is.
int prior_impl(qs_mppi* p, void* stream) {
  return qs::prior_rollout("qs_prior_mppi_rollout", p, p->spec.seed, (const uint64_t*)p->buf[qs::kMppiTick], p->spec.lo,
                           p->spec.hi, stream);
}

int update_impl(qs_mppi* p, hipStream_t st) {
  const UpdateParams P = update_params(p);
  if (p->variant == qs::kMppiPerBlock) {
    hipLaunchKernelGGL(mppi_weights_block_kernel, dim3(p->grids.weights), dim3(qs::kMppiSumThreads), 0, st, P);
    PLANNER_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mppi_sum_block_kernel, dim3(p->grids.sum), dim3(qs::kMppiSumThreads), 0, st, P);
  } else {
    hipLaunchKernelGGL(mppi_weights_thread_kernel, dim3(p->grids.weights), dim3(qs::kMppiThreads), 0, st, P);
    PLANNER_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mppi_sum_thread_kernel, dim3(p->grids.sum), dim3(qs::kMppiThreads), 0, st, P);
  }
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // namespace

namespace {
int create_impl(const char* who, bool per_drone, qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out) {
  qs_dims d;
  if (int rc = qs::planner_check_spec(who, "nominal", h, spec, out, &d)) return rc;
  if (!(spec->lambda >= 0.0) || !std::isfinite(spec->lambda))
    return qs::set_last_error(QS_E_INVALID, std::string(who) + ": lambda must be finite and >= 0 (0: greedy)");
  qs_mppi* p = qs::planner_new<qs_mppi>(who, h, *spec, d);
  if (!p) return QS_E_NOMEM;
  p->per_drone = per_drone;
  const qs::MppiShape shape{p->n, p->C, p->E, p->D, p->A};
  if (per_drone ? !qs::mppi_pd_sizes(shape, p->bytes, &p->ret_agent_bytes) : !qs::mppi_sizes(shape, p->bytes))
    return qs::planner_too_large(who, p);
  const qs::MppiShape ushape = per_drone ? qs::mppi_pd_shape(shape) : shape;   // the update's units and rows
  p->variant = qs::mppi_variant(ushape.E, ushape.C, ushape.D * ushape.A);
  p->grids = qs::mppi_grids(ushape, p->variant);
  if (int rc = qs::planner_alloc(who, p, qs::kMppiCandidates)) return rc;
  *out = p;
  return QS_OK;
}
}  // namespace

extern "C" {

int qs_mppi_create(qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out) {
  return create_impl("qs_mppi_create", false, h, spec, out);
}

int qs_pd_mppi_create(qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out) {
  return create_impl("qs_pd_mppi_create", true, h, spec, out);
}

int qs_pd_mppi_ret_agent(const qs_mppi* p, double** out) { return qs::planner_ret_agent("qs_pd_mppi_ret_agent", p, out); }

int qs_mppi_destroy(qs_mppi* p) { return qs::planner_destroy(p); }

int qs_mppi_buffers(const qs_mppi* p, qs_mppi_bufs* out) {
  if (!p || !out) return qs::set_last_error(QS_E_INVALID, "qs_mppi_buffers: null argument");
  out->nominal = (float*)p->buf[qs::kMppiNominal];
  out->candidates = (float*)p->buf[qs::kMppiCandidates];
  out->ret = (double*)p->buf[qs::kMppiRet];
  out->first_done = (int32_t*)p->buf[qs::kMppiFirstDone];
  out->weights = (double*)p->buf[qs::kMppiWeights];
  out->best = (int32_t*)p->buf[qs::kMppiBest];
  out->action = (float*)p->buf[qs::kMppiAction];
  out->tick = (uint64_t*)p->buf[qs::kMppiTick];
  return QS_OK;
}

int qs_mppi_reset(qs_mppi* p, const float* nominal, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_reset: null planner");
  return qs::planner_reset(p, qs::kMppiNominal, qs::kMppiTick, nominal, (hipStream_t)stream);
}

int qs_mppi_sample(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_sample: null planner");
  return sample_impl(p, (hipStream_t)stream);
}

int qs_mppi_update(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_update: null planner");
  return update_impl(p, (hipStream_t)stream);
}

int qs_value_mppi_set(qs_mppi* p, const qs_value_spec* spec) { return qs::value_attach("qs_value_mppi_set", p, spec); }

int qs_value_mppi_buffers(const qs_mppi* p, float** last_obs, float** value, void** rewards) {
  return qs::value_buffers("qs_value_mppi_buffers", p, last_obs, value, rewards);
}

int qs_value_mppi_score(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_value_mppi_score: null planner");
  if (int rc = qs::planner_ready("qs_value_mppi_score", p)) return rc;
  return qs::value_score(p, p->buf[qs::kMppiRet], p->buf[qs::kMppiFirstDone], stream);
}

int qs_prior_mppi_set(qs_mppi* p, const qs_prior_spec* spec) { return qs::prior_attach("qs_prior_mppi_set", p, spec); }

int qs_prior_mppi_buffers(const qs_mppi* p, float** prior_actions, float** prior_obs) {
  return qs::prior_buffers("qs_prior_mppi_buffers", p, prior_actions, prior_obs);
}

int qs_prior_mppi_rollout(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_prior_mppi_rollout: null planner");
  if (int rc = qs::planner_ready("qs_prior_mppi_rollout", p)) return rc;
  return prior_impl(p, stream);
}

int qs_sampling_mppi_set(qs_mppi* p, const qs_sampling_spec* spec) {
  return qs::sampling_attach("qs_sampling_mppi_set", p, qs::kSamplingMppi, 0, spec);
}

int qs_avoid_mppi_set(qs_mppi* p, const qs_avoid_spec* spec) { return qs::avoid_attach("qs_avoid_mppi_set", p, spec); }

int qs_avoid_mppi_buffers(const qs_mppi* p, double** cost_agent, double** ret_agent) {
  return qs::track_buffers("qs_avoid_mppi_buffers", p, cost_agent, ret_agent);
}

int qs_avoid_mppi_score(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_avoid_mppi_score: null planner");
  if (int rc = qs::planner_ready("qs_avoid_mppi_score", p)) return rc;
  return qs::planner_score(p, p->buf[qs::kMppiRet], p->buf[qs::kMppiFirstDone], stream);
}

int qs_track_mppi_set(qs_mppi* p, const qs_track_spec* spec) { return qs::track_attach("qs_track_mppi_set", p, spec); }

int qs_track_mppi_buffers(const qs_mppi* p, double** cost_agent, double** ret_agent) {
  return qs::track_buffers("qs_track_mppi_buffers", p, cost_agent, ret_agent);
}

int qs_track_mppi_score(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_track_mppi_score: null planner");
  if (int rc = qs::planner_ready("qs_track_mppi_score", p)) return rc;
  return qs::planner_score(p, p->buf[qs::kMppiRet], p->buf[qs::kMppiFirstDone], stream);
}

int qs_mppi_plan(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_plan: null planner");
  if (int rc = qs::planner_ready("qs_mppi_plan", p)) return rc;
  if (p->prior)
    if (int rc = prior_impl(p, stream)) return rc;
  if (int rc = sample_impl(p, (hipStream_t)stream)) return rc;
  if (int rc = qs::value_score(p, p->buf[qs::kMppiRet], p->buf[qs::kMppiFirstDone], stream)) return rc;
  return update_impl(p, (hipStream_t)stream);
}

}  // extern "C"
