// planner_common.h — what the MPPI tick (planner.hip) and the CEM tick
// (planner_cem.hip) share, the sample stage with the particle tick (planner_smc.hip)
// too: the sample kernel and its serial-in-j twin for a sampling spec's correlated
// noise (qs_sampling_*_set, sampling_sizes.h), the penalised score, the row
// reduction of the per-workgroup variants, and the host record with its create /
// destroy / reset / score plumbing.  HIP; included by the planner files only
// (planner_value.hip, the value tail of the score stage, and planner_prior.hip, the
// policy prior, among them).
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include <new>

#include "quadswarm.h"
#include "planner_link.h"
#include "planner_sizes.h"
#include "sampling_sizes.h"
#include "step_kernel.h"   // qs::philox

#define PLANNER_HIP_TRY(expr)                                                                     \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return qs::set_last_error(QS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace qs {

// ---- device ------------------------------------------------------------------------
// Spread is where the sample kernel reads a component's standard deviation from:
// `float at(size_t i, int a) const`, i the element's offset in [n][E][D][A].
template <class Spread>
struct SampleParams {
  const float* mean;         // [n][E][D][A]: the sequence the candidates are drawn round
  float* cand;               // [n][C][E][D][A]
  const uint64_t* tick;
  uint32_t k0, k1, genv0, tag, iter;   // Philox key, global id of env 0, domain tag, iteration
  int n, C, E, D, A;
  float lo, hi;
  Spread spread;
  // The CEM tick's elite memory (a sampling spec with keep > 0; null: none): candidates
  // 1 .. *kept_n are not drawn but copied from kept rows 0 .. *kept_n - 1.
  const float* kept = nullptr;       // [n][keep][E][D][A]
  const int32_t* kept_n = nullptr;   // [1], read on the device: 0 after create / reset, keep from the first refit on
  uint32_t keep = 0;
};

// Whether candidate c > 0 is a kept elite, and then `out` its [A] values of step j,
// bit for bit (they were clipped when they were drawn).  The test on c comes first:
// only the threads of candidates 1 .. keep read the count.
template <class Spread>
__device__ __forceinline__ bool sample_kept(const SampleParams<Spread>& P, uint32_t c, uint32_t have, uint32_t ED, uint32_t ed,
                                            int j, float* out) {
  if (c > have) return false;
  const float* src = P.kept + (((size_t)j * P.keep + (c - 1u)) * ED + ed) * P.A;
  for (int a = 0; a < P.A; ++a) out[a] = src[a];
  return true;
}
// *kept_n held to 0 .. keep (a caller's own bytes must not index past the buffer); 0 without elite memory.
template <class Spread>
__device__ __forceinline__ uint32_t sample_kept_count(const SampleParams<Spread>& P, uint32_t c) {
  if (!P.kept || c > P.keep) return 0u;
  const int32_t have = *P.kept_n;
  return have < 0 ? 0u : ((uint32_t)have > P.keep ? P.keep : (uint32_t)have);
}

// 24-bit uniform in (0, 1]: ln u is finite.
__device__ __forceinline__ float u01_open0(uint32_t x) { return (float)((x >> 8) + 1u) * (1.0f / 16777216.0f); }

// The float32 normals of (tick, env e, candidate c, step j, drone d): one Philox call
// and the Box–Muller pairs the A components use, the others 0.
template <class Spread>
__device__ __forceinline__ void sample_normals(const SampleParams<Spread>& P, uint32_t tick, uint32_t e, uint32_t c, uint32_t j,
                                               uint32_t d, float (&z)[4]) {
  const U4 x = philox(U4{tick, P.genv0 + e, c * 32u + j, (P.tag << 24) | (P.iter << 8) | d}, P.k0, P.k1);
  const float two_pi = 6.283185307179586f;
  z[0] = z[1] = z[2] = z[3] = 0.0f;
  const float r0 = sqrtf(-2.0f * logf(u01_open0(x.x))), a0 = two_pi * u01_open0(x.y);
  z[0] = r0 * cosf(a0);
  if (P.A > 1) z[1] = r0 * sinf(a0);
  if (P.A > 2) {   // (kernel-uniform)
    const float r1 = sqrtf(-2.0f * logf(u01_open0(x.z))), a1 = two_pi * u01_open0(x.w);
    z[2] = r1 * cosf(a1);
    z[3] = r1 * sinf(a1);
  }
}

// One thread per (candidate, env, drone) of step j = blockIdx.y: C · E · D is below
// 2^31 (planner_sizes.h), so the index arithmetic is 32-bit.  Candidate 0 is the
// mean itself.  Only the normals the action components use are formed (the second
// Box–Muller pair from A = 3 on).
template <class Spread>
__global__ __launch_bounds__(kPlannerThreads) void planner_sample_kernel(SampleParams<Spread> P) {
  const uint32_t v = blockIdx.x * (uint32_t)kPlannerThreads + threadIdx.x;
  const uint32_t ED = (uint32_t)P.E * (uint32_t)P.D, per_step = (uint32_t)P.C * ED;
  if (v >= per_step) return;
  const int j = blockIdx.y;
  const uint32_t c = v / ED, ed = v - c * ED, e = ed / (uint32_t)P.D, d = ed - e * (uint32_t)P.D;
  const size_t at = ((size_t)j * ED + ed) * P.A;
  const float* mu = P.mean + at;
  float* out = P.cand + ((size_t)j * per_step + v) * P.A;
  if (c == 0) {
    for (int a = 0; a < P.A; ++a) out[a] = mu[a];
    return;
  }
  if (sample_kept(P, c, sample_kept_count(P, c), ED, ed, j, out)) return;
  const uint32_t tick = (uint32_t)*P.tick;
  float z[4];
  sample_normals(P, tick, e, c, (uint32_t)j, d, z);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a >= P.A) break;
    const float sg = P.spread.at(at, a);
    const float val = sg == 0.0f ? mu[a] : mu[a] + sg * z[a];
    out[a] = fminf(fmaxf(val, P.lo), P.hi);
  }
}

// The sample kernel of a planner with a sampling spec that has a non-zero rho
// (qs_sampling_*_set): the noise of component a is the AR(1) sequence eps_0 = xi_0,
// eps_j = rho_a · eps_{j-1} + s_a · xi_j over the steps of the launch, xi_j exactly the
// normal planner_sample_kernel forms for step j (the same Philox counter, one call
// per step).  One thread per (candidate, env, drone) walks j = 0 .. n - 1 with eps in
// registers, so the grid is x of the (sample, n) grid this launch replaces; at every
// j the wave's stores are as coalesced as that kernel's.  The two products and the sum
// are separate float32 roundings (never a fused multiply-add); a component with
// rho = 0 takes xi as it is, with no arithmetic, so its bytes are that kernel's.
template <class Spread>
struct SampleArParams {
  SampleParams<Spread> S;
  float rho[4], scale[4];    // scale[a] = sampling_scale(rho[a]), formed on the host
};

template <class Spread>
__global__ __launch_bounds__(kPlannerThreads) void planner_sample_ar_kernel(SampleArParams<Spread> Q) {
  const SampleParams<Spread>& P = Q.S;
  const uint32_t v = blockIdx.x * (uint32_t)kPlannerThreads + threadIdx.x;
  const uint32_t ED = (uint32_t)P.E * (uint32_t)P.D, per_step = (uint32_t)P.C * ED;
  if (v >= per_step) return;
  const uint32_t c = v / ED, ed = v - c * ED, e = ed / (uint32_t)P.D, d = ed - e * (uint32_t)P.D;
  if (c == 0) {
    for (int j = 0; j < P.n; ++j) {
      const float* mu = P.mean + ((size_t)j * ED + ed) * P.A;
      float* out = P.cand + ((size_t)j * per_step + v) * P.A;
      for (int a = 0; a < P.A; ++a) out[a] = mu[a];
    }
    return;
  }
  if (const uint32_t have = sample_kept_count(P, c)) {
    if (c <= have) {
      for (int j = 0; j < P.n; ++j) (void)sample_kept(P, c, have, ED, ed, j, P.cand + ((size_t)j * per_step + v) * P.A);
      return;
    }
  }
  const uint32_t tick = (uint32_t)*P.tick;
  float eps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int j = 0; j < P.n; ++j) {
    const size_t at = ((size_t)j * ED + ed) * P.A;
    const float* mu = P.mean + at;
    float* out = P.cand + ((size_t)j * per_step + v) * P.A;
    float z[4];
    sample_normals(P, tick, e, c, (uint32_t)j, d, z);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= P.A) break;
      eps[a] = (j == 0 || Q.rho[a] == 0.0f) ? z[a] : __fadd_rn(__fmul_rn(Q.rho[a], eps[a]), __fmul_rn(Q.scale[a], z[a]));
      const float sg = P.spread.at(at, a);
      const float val = sg == 0.0f ? mu[a] : mu[a] + sg * eps[a];
      out[a] = fminf(fmaxf(val, P.lo), P.hi);
    }
  }
}

// A candidate's return, less the penalty where it ends an episode inside the n steps.
// `ret` is [C][units] and ce = c · units + u; first_done is [C][units / fd_div]
// and read at ce / fd_div.  Env-level planning has fd_div = 1 (a unit is an env);
// per-drone planning has units = E · D agents and fd_div = D, so agent (e, d) of
// candidate c reads ret_agent[c][e][d] and its env's first_done[c][e].
__device__ __forceinline__ double penalised_score(const double* ret, const int32_t* first_done, int n, double penalty,
                                                  int fd_div, size_t ce) {
  const size_t fd = fd_div == 1 ? ce : ce / (size_t)fd_div;
  return ret[ce] - (first_done[fd] < n ? penalty : 0.0);
}
// ... from a kernel's parameter record that holds ret, first_done, n, penalty and fd_div.
template <class Params>
__device__ __forceinline__ double score_of(const Params& P, size_t ce) {
  return penalised_score(P.ret, P.first_done, P.n, P.penalty, P.fd_div, ce);
}

// The sums over a kPlannerBlockThreads workgroup of `acc` per component
// k = tid mod rowp, left in part[0 .. rowp) (part holds kPlannerBlockThreads
// doubles).  rowp is a power of two, so the lanes of one component sit rowp apart
// in a wave: an xor tree over the offsets 32 .. rowp sums them, then the partials
// (one per wave, or one per group where a row spans whole waves) meet in an LDS
// tree, whose last step ends in a barrier.
__device__ __forceinline__ void block_row_reduce(double acc, double* part, int tid, int rowp) {
  const int lane = tid & 63, wave = tid >> 6;
  int parts;
  if (rowp <= 64) {
    for (int off = 32; off >= rowp; off >>= 1) acc += __shfl_xor(acc, off, 64);
    parts = kPlannerBlockThreads / 64;
    if (lane < rowp) part[wave * rowp + lane] = acc;
  } else {
    parts = kPlannerBlockThreads / rowp;
    part[tid] = acc;   // = part[g * rowp + k]
  }
  __syncthreads();
  for (int s = parts >> 1; s >= 1; s >>= 1) {
    if (tid < s * rowp) part[tid] += part[tid + s * rowp];
    __syncthreads();
  }
}

// ---- host --------------------------------------------------------------------------
struct ValueState;   // planner_value.hip: the attached value's spec copy and buffers
struct PriorState;   // planner_prior.hip: the attached policy prior's spec copy, branch set and buffers
struct TrackState;   // planner_track.hip: the attached tracking spec's copy and buffers

// What a planner holds once a sampling spec is attached (qs_sampling_*_set).
struct SamplingState {
  qs_sampling_spec spec;
  float scale[4];            // sampling_scale(rho[a])
  bool correlated;           // some rho[a], a < A, is not 0: the serial-in-j sample kernel runs
  int keep;                  // CEM: the elites carried over (0: none, and no buffers)
  float* kept;               // [n][keep][E][D][A]
  int32_t* kept_n;           // [1]: rows of `kept` the next sample injects
  uint64_t kept_bytes;
};

// What qs_mppi and qs_cem both are.  The derived records add `spec`, `variant`,
// `grids`, `bytes[]` and `buf[]`.
struct PlannerBase {
  qs_handle* h = nullptr;
  HandleInfo info;
  int n, C, E, D, A;
  std::vector<const float*> steps;   // candidates' n step pointers, the host array qs_score reads
  // Per-drone mode (qs_pd_*_create): every drone weighs the candidates by its own
  // return.  The update / refit kernels then run over E · D units with rows of A
  // components, which is the memory they index anyway, and score a unit from
  // ret_agent and its env's first_done.
  bool per_drone = false;
  void* ret_agent = nullptr;         // [C][E][D] doubles, per-drone mode only
  uint64_t ret_agent_bytes = 0;
  ValueState* value = nullptr;       // qs_value_mppi_set / qs_value_cem_set; null: the plain score
  PriorState* prior = nullptr;       // qs_prior_mppi_set / qs_prior_cem_set; null: every candidate is sampled
  SamplingState* sampling = nullptr; // qs_sampling_*_set; null: white noise and no elite memory
  TrackState* track = nullptr;       // qs_track_*_set / qs_avoid_*_set; null: the task's reward alone
  int units() const { return per_drone ? E * D : E; }      // what the kernels take for envs
  int row() const { return per_drone ? A : D * A; }        // components of a unit's row
  int fd_div() const { return per_drone ? D : 1; }         // units per entry of first_done
  const double* scores(const void* ret) const { return (const double*)(per_drone ? ret_agent : ret); }
};

// The checks every planner spec goes through (`who`: the entry point, `centre`:
// what candidate 0 is); fills `d`.
template <class Spec>
int planner_check_spec(const char* who, const char* centre, qs_handle* h, const Spec* spec, const void* out, qs_dims* d) {
  const std::string w = std::string(who) + ": ";
  if (!h || !spec || !out) return set_last_error(QS_E_INVALID, w + "null argument");
  const int depth = qs_score_depth(h);
  if (depth < 1)
    return set_last_error(QS_E_INVALID, w + "this handle cannot score (qs_score_depth = 0): a layout whose "
                                            "reset draws can be rejected, or a Flock / Meetup / LeaderFollower task");
  if (spec->horizon < 1 || spec->horizon > depth)
    return set_last_error(QS_E_INVALID, w + "horizon = " + std::to_string(spec->horizon) +
                                            " is outside 1 .. qs_score_depth = " + std::to_string(depth));
  if (spec->candidates < 2)
    return set_last_error(QS_E_INVALID, w + "candidates must be >= 2 (candidate 0 is the " + centre + " itself)");
  if (!(spec->lo < spec->hi) || !std::isfinite(spec->lo) || !std::isfinite(spec->hi))
    return set_last_error(QS_E_INVALID, w + "lo must be below hi, both finite");
  if (int rc = qs_get_dims(h, d)) return rc;
  for (int a = 0; a < d->act_dim && a < 4; ++a)
    if (!(spec->sigma[a] >= 0.0f) || !std::isfinite(spec->sigma[a]))
      return set_last_error(QS_E_INVALID, w + "sigma[" + std::to_string(a) + "] must be finite and >= 0");
  if (!(spec->done_penalty >= 0.0) || !std::isfinite(spec->done_penalty))
    return set_last_error(QS_E_INVALID, w + "done_penalty must be finite and >= 0");
  return QS_OK;
}

// A fresh record with its shape and its buffer pointers cleared; null (and the error set) without memory.
template <class T, class Spec>
T* planner_new(const char* who, qs_handle* h, const Spec& spec, const qs_dims& d) {
  T* p = new (std::nothrow) T;
  if (!p) {
    set_last_error(QS_E_NOMEM, std::string(who) + ": out of host memory");
    return nullptr;
  }
  p->h = h;
  p->spec = spec;
  handle_info(h, &p->info);
  p->n = spec.horizon; p->C = spec.candidates; p->E = d.num_envs; p->D = d.num_drones; p->A = d.act_dim;
  for (void*& b : p->buf) b = nullptr;
  return p;
}

// The refusal of a shape *_sizes turns down; deletes the record.
template <class T>
int planner_too_large(const char* who, T* p) {
  delete p;
  return set_last_error(QS_E_INVALID, std::string(who) + ": candidates * num_envs * num_drones is too large (the 32-bit "
                                                         "offsets of qs_score, at most 2^27 candidates)");
}

// The value tail (planner_value.hip).  value_attach copies the spec and allocates
// last_obs / value / rewards (a null spec detaches); value_score is the score stage:
// planner_score, and with a value attached the qs_score launch that also names the
// last obs and the per-step rewards, then the tail.
void value_release(PlannerBase* p);
int value_attach(const char* who, PlannerBase* p, const qs_value_spec* spec);
int value_buffers(const char* who, const PlannerBase* p, float** last_obs, float** value, void** rewards);
int value_score(PlannerBase* p, void* ret, void* first_done, void* stream);

// The policy prior (planner_prior.hip).  prior_attach copies the spec, creates the
// planner's branch set of `count` candidates and allocates prior_actions /
// prior_obs (a null spec detaches); prior_rollout is the prior stage: fork, then
// per step the actor launch and, but for the last step, a one-step advance;
// prior_inject copies prior_actions over the last `count` candidates of every
// step, and launches nothing without a prior.
void prior_release(PlannerBase* p);
int prior_attach(const char* who, PlannerBase* p, const qs_prior_spec* spec);
int prior_buffers(const char* who, const PlannerBase* p, float** prior_actions, float** prior_obs);
int prior_rollout(const char* who, PlannerBase* p, uint64_t seed, const uint64_t* tick, float lo, float hi, void* stream);
int prior_inject(PlannerBase* p, float* candidates, void* stream);
int prior_count(const PlannerBase* p);   // the attached prior's candidates per env, 0 without one

// The tracking cost (planner_track.hip).  track_attach copies the spec and allocates
// cost_agent, and ret_agent for an env-level planner (a null spec detaches; refused
// next to a value tail, as value_attach refuses next to tracking); track_score is the
// score stage with a spec attached: qs_track_score, then the fold launch.
void track_release(PlannerBase* p);
int track_attach(const char* who, PlannerBase* p, const qs_track_spec* spec);
bool track_attached(const PlannerBase* p);
// The separation and obstacle terms (planner_track.hip): avoid_attach copies the spec
// next to the tracking one, or on its own, and shares its buffers and its score stage.
int avoid_attach(const char* who, PlannerBase* p, const qs_avoid_spec* spec);
bool avoid_attached(const PlannerBase* p);
int track_buffers(const char* who, const PlannerBase* p, double** cost_agent, double** ret_agent);
int track_score(PlannerBase* p, void* ret, void* first_done, void* stream);

// The sampling spec (qs_sampling_*_set; the arithmetic is sampling_sizes.h).
inline void sampling_release(PlannerBase* p) {
  if (!p->sampling) return;
  if (p->sampling->kept) (void)hipFree(p->sampling->kept);
  if (p->sampling->kept_n) (void)hipFree(p->sampling->kept_n);
  delete p->sampling;
  p->sampling = nullptr;
}

inline int sampling_refuse(const char* who, SamplingRefusal r, const qs_sampling_spec* s, const SamplingShape& shape) {
  const std::string w = std::string(who) + ": ";
  switch (r) {
    case kSamplingRho:
      return set_last_error(QS_E_INVALID, w + "rho must be in [0, 1) for each of the " + std::to_string((long long)shape.A) +
                                              " action components");
    case kSamplingReserved:
      return set_last_error(QS_E_INVALID, w + "reserved = " + std::to_string(s->reserved) + " must be 0");
    case kSamplingKeepNeg:
      return set_last_error(QS_E_INVALID, w + "keep = " + std::to_string(s->keep) + " is negative");
    case kSamplingKeepKind:
      return set_last_error(QS_E_INVALID, w + "keep = " + std::to_string(s->keep) +
                                              " must be 0 here: only the CEM tick has elites to keep (qs_sampling_cem_set)");
    case kSamplingKeepElites:
      return set_last_error(QS_E_INVALID, w + "keep = " + std::to_string(s->keep) + " is above elites = " +
                                              std::to_string((long long)shape.K));
    case kSamplingSlots:
      return set_last_error(QS_E_INVALID, w + "1 + keep + the prior's count = 1 + " + std::to_string(s->keep) + " + " +
                                              std::to_string((long long)shape.prior) + " is above candidates = " +
                                              std::to_string((long long)shape.C) +
                                              " (the mean, the kept elites and the prior's rollouts each need their own slots)");
    case kSamplingOffsets:
      return set_last_error(QS_E_INVALID, w + "keep * num_envs * num_drones * act_dim * 4 bytes of a step of kept is past "
                                              "the 32-bit offsets");
    default:
      return QS_OK;
  }
}

// Copies the spec and, with keep > 0, allocates and zeroes kept / kept_n (a null spec
// detaches).  K: the planner's elites (CEM), 0 otherwise.  A refusal leaves the planner,
// and a spec attached earlier, as they were.
inline int sampling_attach(const char* who, PlannerBase* p, SamplingKind kind, int K, const qs_sampling_spec* spec) {
  if (!p) return set_last_error(QS_E_INVALID, std::string(who) + ": null planner");
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (!spec) {   // detach; the work in flight may still read the buffers
    if (p->sampling && p->sampling->kept) PLANNER_HIP_TRY(hipDeviceSynchronize());
    sampling_release(p);
    return QS_OK;
  }
  const SamplingShape shape{kind, p->n, p->C, K, prior_count(p), p->E, p->D, p->A};
  SamplingSpecShape v;
  for (int a = 0; a < 4; ++a) v.rho[a] = spec->rho[a];
  v.keep = spec->keep;
  v.reserved = spec->reserved;
  if (const SamplingRefusal r = sampling_refusal(v, shape)) return sampling_refuse(who, r, spec, shape);
  SamplingState* s = new (std::nothrow) SamplingState;
  if (!s) return set_last_error(QS_E_NOMEM, std::string(who) + ": out of host memory");
  s->spec = *spec;
  for (int a = 0; a < 4; ++a) {
    if (a >= p->A) s->spec.rho[a] = 0.0f;   // (not read; the kernel's record holds numbers)
    s->scale[a] = sampling_scale(s->spec.rho[a]);
  }
  s->correlated = sampling_correlated(s->spec.rho, p->A);
  s->keep = spec->keep;
  s->kept = nullptr;
  s->kept_n = nullptr;
  s->kept_bytes = 0;
  if (s->keep > 0) {
    (void)sampling_kept_bytes(p->n, s->keep, p->E, p->D, p->A, &s->kept_bytes);   // (sampling_refusal has accepted it)
    hipError_t e = hipMalloc((void**)&s->kept, s->kept_bytes);
    if (e == hipSuccess) e = hipMemset(s->kept, 0, s->kept_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&s->kept_n, 4);
    if (e == hipSuccess) e = hipMemset(s->kept_n, 0, 4);
    if (e != hipSuccess) {
      if (s->kept) (void)hipFree(s->kept);
      if (s->kept_n) (void)hipFree(s->kept_n);
      delete s;
      return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
  }
  if (p->sampling) {   // replaced; the work in flight may still read the old buffers
    if (p->sampling->kept) (void)hipDeviceSynchronize();
    sampling_release(p);
  }
  p->sampling = s;
  return QS_OK;
}

// The sample launch of every planner: planner_sample_kernel over a (grid_x, n) grid,
// or with a correlated sampling spec planner_sample_ar_kernel over grid_x workgroups.
template <class Spread>
int planner_launch_sample(const PlannerBase* p, const SampleParams<Spread>& P, uint32_t grid_x, hipStream_t st) {
  const SamplingState* s = p->sampling;
  if (s && s->correlated) {
    SampleArParams<Spread> Q;
    Q.S = P;
    for (int a = 0; a < 4; ++a) { Q.rho[a] = s->spec.rho[a]; Q.scale[a] = s->scale[a]; }
    hipLaunchKernelGGL(planner_sample_ar_kernel<Spread>, dim3(grid_x), dim3(kPlannerThreads), 0, st, Q);
  } else {
    hipLaunchKernelGGL(planner_sample_kernel<Spread>, dim3(grid_x, (uint32_t)P.n), dim3(kPlannerThreads), 0, st, P);
  }
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

template <class T>
void planner_free(T* p) {
  for (void* b : p->buf)
    if (b) (void)hipFree(b);
  if (p->ret_agent) (void)hipFree(p->ret_agent);
  value_release(p);
  prior_release(p);
  sampling_release(p);
  track_release(p);
}

// Allocates and zeroes every buffer of p->bytes (and ret_agent where
// ret_agent_bytes is set) and points `steps` into buffer `candidates`; on failure
// frees what it made and deletes the record.
template <class T>
int planner_alloc(const char* who, T* p, int candidates) {
  constexpr int kBufs = sizeof(p->buf) / sizeof(p->buf[0]);
  hipError_t e = hipSetDevice(p->info.device);
  for (int i = 0; i < kBufs && e == hipSuccess; ++i) {
    e = hipMalloc(&p->buf[i], p->bytes[i]);
    if (e == hipSuccess) e = hipMemset(p->buf[i], 0, p->bytes[i]);
  }
  if (e == hipSuccess && p->ret_agent_bytes != 0) {
    e = hipMalloc(&p->ret_agent, p->ret_agent_bytes);
    if (e == hipSuccess) e = hipMemset(p->ret_agent, 0, p->ret_agent_bytes);
  }
  if (e != hipSuccess) {
    planner_free(p);
    delete p;
    return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  }
  const size_t step = (size_t)(p->bytes[candidates] / 4u / (uint64_t)p->n);
  for (int j = 0; j < p->n; ++j) p->steps.push_back((const float*)p->buf[candidates] + (size_t)j * step);
  return QS_OK;
}

template <class T>
int planner_destroy(T* p) {
  if (!p) return QS_OK;
  (void)hipSetDevice(p->info.device);   // teardown: best effort
  planner_free(p);
  delete p;
  return QS_OK;
}

// Buffer `seq` becomes a copy of `src` (device memory; null: zeros) and the tick 0.
template <class T>
int planner_reset(T* p, int seq, int tick, const float* src, hipStream_t st) {
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (src)
    PLANNER_HIP_TRY(hipMemcpyAsync(p->buf[seq], src, p->bytes[seq], hipMemcpyDeviceToDevice, st));
  else
    PLANNER_HIP_TRY(hipMemsetAsync(p->buf[seq], 0, p->bytes[seq], st));
  PLANNER_HIP_TRY(hipMemsetAsync(p->buf[tick], 0, p->bytes[tick], st));
  return QS_OK;
}

// plan()'s gate: the handle's state as it is now, refused before qs_reset.
inline int planner_ready(const char* who, PlannerBase* p) {
  handle_info(p->h, &p->info);
  if (!p->info.reset_done) return set_last_error(QS_E_STATE, std::string(who) + ": call qs_reset first");
  return QS_OK;
}

// Scores the candidates from the handle's current state into ret / first_done
// (and, in per-drone mode, ret_agent); with a tracking spec attached, the folded
// objective (track_score).
inline int planner_score(PlannerBase* p, void* ret, void* first_done, void* stream) {
  if (p->track) return track_score(p, ret, first_done, stream);
  const qs_score_out so{ret, (int32_t*)first_done};
  if (p->per_drone)
    return qs_score_agents(p->h, p->n, p->C, p->steps.data(), nullptr, &so, (double*)p->ret_agent, stream);
  return qs_score(p->h, p->n, p->C, p->steps.data(), nullptr, &so, stream);
}

// qs_pd_*_ret_agent.
inline int planner_ret_agent(const char* who, const PlannerBase* p, double** out) {
  if (!p || !out) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  if (!p->per_drone)
    return set_last_error(QS_E_INVALID, std::string(who) + ": this is an env-level planner (it has no ret_agent; "
                                                           "create it with the qs_pd_ entry point)");
  *out = (double*)p->ret_agent;
  return QS_OK;
}

}  // namespace qs
