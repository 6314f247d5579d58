// planner.hip — the MPPI planner tick on top of qs_score (include/quadswarm.h,
// qs_mppi_*; DESIGN.md §4a "Planner tick").
//
// Three kernels round the one qs_score launch: mppi_sample_kernel perturbs the
// nominal sequence into C candidates, mppi_weights_* turns qs_score's ret /
// first_done into softmax weights per env, and mppi_sum_* folds the candidates
// back into the nominal, shifted by one step.  Everything per env is summed in
// double in a fixed order (no atomics), the tick counter lives on the device, and
// nothing is read back, so a tick can be captured and replayed.  The host
// arithmetic (sizes, variant, grids) is planner_sizes.h.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include <new>

#include "quadswarm.h"
#include "planner_link.h"
#include "planner_sizes.h"
#include "step_kernel.h"   // qs::philox

namespace {

#define MPPI_HIP_TRY(expr)                                                                        \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return qs::set_last_error(QS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

struct SampleParams {
  const float* nominal;      // [n][E][D][A]
  float* cand;               // [n][C][E][D][A]
  const uint64_t* tick;
  uint32_t k0, k1, genv0;
  int n, C, E, D, A;
  float sigma[4];
  float lo, hi;
};

struct UpdateParams {
  const float* cand;         // [n][C][E][D][A]
  const double* ret;         // [C][E]
  const int32_t* first_done; // [C][E]
  double* w;                 // [C][E]
  int32_t* best;             // [E]
  float* nominal;            // [n][E][D][A]
  float* action;             // [E][D][A]
  uint64_t* tick;
  double lambda, penalty;
  int n, C, E, row, rowp;    // row = D · A, rowp = the power of two >= row
};

// 24-bit uniform in (0, 1]: ln u is finite.
__device__ __forceinline__ float u01_open0(uint32_t x) { return (float)((x >> 8) + 1u) * (1.0f / 16777216.0f); }

// One thread per (candidate, env, drone) of step j = blockIdx.y: C · E · D is below
// 2^31 (planner_sizes.h), so the index arithmetic is 32-bit.  Only the normals the
// action components use are formed (the second Box–Muller pair from A = 3 on).
__global__ __launch_bounds__(qs::kMppiThreads) void mppi_sample_kernel(SampleParams P) {
  const uint32_t v = blockIdx.x * (uint32_t)qs::kMppiThreads + threadIdx.x;
  const uint32_t ED = (uint32_t)P.E * (uint32_t)P.D, per_step = (uint32_t)P.C * ED;
  if (v >= per_step) return;
  const int j = blockIdx.y;
  const uint32_t c = v / ED, ed = v - c * ED, e = ed / (uint32_t)P.D, d = ed - e * (uint32_t)P.D;
  const float* nom = P.nominal + ((size_t)j * ED + ed) * P.A;
  float* out = P.cand + ((size_t)j * per_step + v) * P.A;
  if (c == 0) {
    for (int a = 0; a < P.A; ++a) out[a] = nom[a];
    return;
  }
  const uint32_t tick = (uint32_t)*P.tick;
  const qs::U4 x = qs::philox(qs::U4{tick, P.genv0 + e, c * 32u + (uint32_t)j, ((uint32_t)qs::kMppiTag << 24) | d},
                              P.k0, P.k1);
  const float two_pi = 6.283185307179586f;
  float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const float r0 = sqrtf(-2.0f * logf(u01_open0(x.x))), a0 = two_pi * u01_open0(x.y);
  z[0] = r0 * cosf(a0);
  if (P.A > 1) z[1] = r0 * sinf(a0);
  if (P.A > 2) {   // (kernel-uniform)
    const float r1 = sqrtf(-2.0f * logf(u01_open0(x.z))), a1 = two_pi * u01_open0(x.w);
    z[2] = r1 * cosf(a1);
    z[3] = r1 * sinf(a1);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a >= P.A) break;
    const float sg = P.sigma[a];
    const float val = sg == 0.0f ? nom[a] : nom[a] + sg * z[a];
    out[a] = fminf(fmaxf(val, P.lo), P.hi);
  }
}

__device__ __forceinline__ double score_of(const UpdateParams& P, size_t ce) {
  return P.ret[ce] - (P.first_done[ce] < P.n ? P.penalty : 0.0);
}
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
// strides over c by the group count.  rowp is a power of two, so the lanes of one
// component sit rowp apart in a wave: an xor tree over the offsets 32 .. rowp
// sums them, then the partials (one per wave, or one per group where a row
// spans whole waves) meet in an LDS tree.
__global__ __launch_bounds__(qs::kMppiSumThreads) void mppi_sum_block_kernel(UpdateParams P) {
  __shared__ double part[qs::kMppiSumThreads];   // [partials][rowp], at most 16 · 64 or 1024 / rowp · rowp
  const int e = blockIdx.x % P.E, j = blockIdx.x / P.E;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  int parts;
  if (rowp <= 64) {
    for (int off = 32; off >= rowp; off >>= 1) acc += __shfl_xor(acc, off, 64);
    parts = qs::kMppiSumThreads / 64;
    if (lane < rowp) part[wave * rowp + lane] = acc;
  } else {
    parts = G;
    part[tid] = acc;   // = part[g * rowp + k]
  }
  __syncthreads();
  for (int s = parts >> 1; s >= 1; s >>= 1) {
    if (tid < s * rowp) part[tid] += part[tid + s * rowp];
    __syncthreads();
  }
  if (tid < P.row) store_new(P, j, e, tid, (float)part[tid]);
}

}  // namespace

struct qs_mppi {
  qs_handle* h = nullptr;
  qs_mppi_spec spec;
  qs_dims dims;
  qs::HandleInfo info;
  qs::MppiShape shape;
  qs::MppiVariant variant;
  qs::MppiGrids grids;
  uint64_t bytes[qs::kMppiBufs];
  void* buf[qs::kMppiBufs];
  std::vector<const float*> steps;   // candidates' n step pointers, the host array qs_score reads
};

namespace {

int set_device(const qs_mppi* p) {
  MPPI_HIP_TRY(hipSetDevice(p->info.device));
  return QS_OK;
}

UpdateParams update_params(const qs_mppi* p) {
  UpdateParams P;
  P.cand = (const float*)p->buf[qs::kMppiCandidates];
  P.ret = (const double*)p->buf[qs::kMppiRet];
  P.first_done = (const int32_t*)p->buf[qs::kMppiFirstDone];
  P.w = (double*)p->buf[qs::kMppiWeights];
  P.best = (int32_t*)p->buf[qs::kMppiBest];
  P.nominal = (float*)p->buf[qs::kMppiNominal];
  P.action = (float*)p->buf[qs::kMppiAction];
  P.tick = (uint64_t*)p->buf[qs::kMppiTick];
  P.lambda = p->spec.lambda;
  P.penalty = p->spec.done_penalty;
  P.n = (int)p->shape.n; P.C = (int)p->shape.C; P.E = (int)p->shape.E;
  P.row = (int)(p->shape.D * p->shape.A);
  P.rowp = qs::mppi_row_pow2(P.row);
  return P;
}

int sample_impl(qs_mppi* p, hipStream_t st) {
  SampleParams P;
  P.nominal = (const float*)p->buf[qs::kMppiNominal];
  P.cand = (float*)p->buf[qs::kMppiCandidates];
  P.tick = (const uint64_t*)p->buf[qs::kMppiTick];
  P.k0 = (uint32_t)p->spec.seed; P.k1 = (uint32_t)(p->spec.seed >> 32);
  P.genv0 = (uint32_t)p->info.env_offset;
  P.n = (int)p->shape.n; P.C = (int)p->shape.C; P.E = (int)p->shape.E; P.D = (int)p->shape.D; P.A = (int)p->shape.A;
  for (int a = 0; a < 4; ++a) P.sigma[a] = p->spec.sigma[a];
  P.lo = p->spec.lo; P.hi = p->spec.hi;
  hipLaunchKernelGGL(mppi_sample_kernel, dim3(p->grids.sample, (uint32_t)p->shape.n), dim3(qs::kMppiThreads), 0, st, P);
  MPPI_HIP_TRY(hipGetLastError());
  return QS_OK;
}

int update_impl(qs_mppi* p, hipStream_t st) {
  const UpdateParams P = update_params(p);
  if (p->variant == qs::kMppiPerBlock) {
    hipLaunchKernelGGL(mppi_weights_block_kernel, dim3(p->grids.weights), dim3(qs::kMppiSumThreads), 0, st, P);
    MPPI_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mppi_sum_block_kernel, dim3(p->grids.sum), dim3(qs::kMppiSumThreads), 0, st, P);
  } else {
    hipLaunchKernelGGL(mppi_weights_thread_kernel, dim3(p->grids.weights), dim3(qs::kMppiThreads), 0, st, P);
    MPPI_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mppi_sum_thread_kernel, dim3(p->grids.sum), dim3(qs::kMppiThreads), 0, st, P);
  }
  MPPI_HIP_TRY(hipGetLastError());
  return QS_OK;
}

void free_bufs(qs_mppi* p) {
  for (void* b : p->buf)
    if (b) (void)hipFree(b);
}

}  // namespace

extern "C" {

int qs_mppi_create(qs_handle* h, const qs_mppi_spec* spec, qs_mppi** out) {
  using qs::set_last_error;
  if (!h || !spec || !out) return set_last_error(QS_E_INVALID, "qs_mppi_create: null argument");
  const int depth = qs_score_depth(h);
  if (depth < 1)
    return set_last_error(QS_E_INVALID, "qs_mppi_create: this handle cannot score (qs_score_depth = 0): a layout whose "
                                        "reset draws can be rejected, or a Flock / Meetup / LeaderFollower task");
  if (spec->horizon < 1 || spec->horizon > depth)
    return set_last_error(QS_E_INVALID, "qs_mppi_create: horizon = " + std::to_string(spec->horizon) +
                                            " is outside 1 .. qs_score_depth = " + std::to_string(depth));
  if (spec->candidates < 2)
    return set_last_error(QS_E_INVALID, "qs_mppi_create: candidates must be >= 2 (candidate 0 is the nominal itself)");
  if (!(spec->lo < spec->hi) || !std::isfinite(spec->lo) || !std::isfinite(spec->hi))
    return set_last_error(QS_E_INVALID, "qs_mppi_create: lo must be below hi, both finite");
  qs_dims d;
  if (int rc = qs_get_dims(h, &d)) return rc;
  for (int a = 0; a < d.act_dim && a < 4; ++a)
    if (!(spec->sigma[a] >= 0.0f) || !std::isfinite(spec->sigma[a]))
      return set_last_error(QS_E_INVALID, "qs_mppi_create: sigma[" + std::to_string(a) + "] must be finite and >= 0");
  if (!(spec->lambda >= 0.0) || !std::isfinite(spec->lambda))
    return set_last_error(QS_E_INVALID, "qs_mppi_create: lambda must be finite and >= 0 (0: greedy)");
  if (!(spec->done_penalty >= 0.0) || !std::isfinite(spec->done_penalty))
    return set_last_error(QS_E_INVALID, "qs_mppi_create: done_penalty must be finite and >= 0");
  qs_mppi* p = new (std::nothrow) qs_mppi;
  if (!p) return set_last_error(QS_E_NOMEM, "qs_mppi_create: out of host memory");
  p->h = h;
  p->spec = *spec;
  p->dims = d;
  qs::handle_info(h, &p->info);
  p->shape = qs::MppiShape{spec->horizon, spec->candidates, d.num_envs, d.num_drones, d.act_dim};
  for (void*& b : p->buf) b = nullptr;
  if (!qs::mppi_sizes(p->shape, p->bytes)) {
    delete p;
    return set_last_error(QS_E_INVALID, "qs_mppi_create: candidates * num_envs * num_drones is too large (the 32-bit "
                                        "offsets of qs_score, at most 2^27 candidates)");
  }
  p->variant = qs::mppi_variant(p->shape.E, p->shape.C, p->shape.D * p->shape.A);
  p->grids = qs::mppi_grids(p->shape, p->variant);
  hipError_t e = hipSetDevice(p->info.device);
  for (int i = 0; i < qs::kMppiBufs && e == hipSuccess; ++i) {
    e = hipMalloc(&p->buf[i], p->bytes[i]);
    if (e == hipSuccess) e = hipMemset(p->buf[i], 0, p->bytes[i]);
  }
  if (e != hipSuccess) {
    free_bufs(p);
    delete p;
    return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP,
                          std::string("qs_mppi_create: ") + hipGetErrorString(e));
  }
  const size_t step = (size_t)(p->bytes[qs::kMppiCandidates] / 4u / (uint64_t)p->shape.n);
  for (int j = 0; j < p->shape.n; ++j) p->steps.push_back((const float*)p->buf[qs::kMppiCandidates] + (size_t)j * step);
  *out = p;
  return QS_OK;
}

int qs_mppi_destroy(qs_mppi* p) {
  if (!p) return QS_OK;
  (void)hipSetDevice(p->info.device);   // teardown: best effort
  free_bufs(p);
  delete p;
  return QS_OK;
}

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
  hipStream_t st = (hipStream_t)stream;
  if (int rc = set_device(p)) return rc;
  if (nominal)
    MPPI_HIP_TRY(hipMemcpyAsync(p->buf[qs::kMppiNominal], nominal, p->bytes[qs::kMppiNominal], hipMemcpyDeviceToDevice, st));
  else
    MPPI_HIP_TRY(hipMemsetAsync(p->buf[qs::kMppiNominal], 0, p->bytes[qs::kMppiNominal], st));
  MPPI_HIP_TRY(hipMemsetAsync(p->buf[qs::kMppiTick], 0, p->bytes[qs::kMppiTick], st));
  return QS_OK;
}

int qs_mppi_sample(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_sample: null planner");
  return sample_impl(p, (hipStream_t)stream);
}

int qs_mppi_update(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_update: null planner");
  return update_impl(p, (hipStream_t)stream);
}

int qs_mppi_plan(qs_mppi* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_mppi_plan: null planner");
  qs::handle_info(p->h, &p->info);
  if (!p->info.reset_done) return qs::set_last_error(QS_E_STATE, "qs_mppi_plan: call qs_reset first");
  if (int rc = sample_impl(p, (hipStream_t)stream)) return rc;
  const qs_score_out so{p->buf[qs::kMppiRet], (int32_t*)p->buf[qs::kMppiFirstDone]};
  if (int rc = qs_score(p->h, (int)p->shape.n, (int)p->shape.C, p->steps.data(), nullptr, &so, stream)) return rc;
  return update_impl(p, (hipStream_t)stream);
}

}  // extern "C"
