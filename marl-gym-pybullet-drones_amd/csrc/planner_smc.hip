// planner_smc.hip — the particle (sequential Monte Carlo) planner tick on top of a
// branch set (include/quadswarm.h, qs_smc_*; DESIGN.md §4a "Particle tick").
//
// A tick is begin (fork the planner's branch set), then per segment s of at most L
// steps: sample (planner_sample_kernel, shared with the MPPI and CEM ticks, over
// the segment's steps; planner_sample_ar_kernel with a correlated sampling spec,
// qs_sampling_smc_set, its recurrence restarting at the segment), advance (qs_branch_advance) and resample (smc_weigh_*:
// weights, effective sample size and, where that is low, systematic resampling
// into parents[s]; then qs_branch_select), then finish: the final weights, the
// ancestry trace back through parents (smc_trace_kernel) and the weighted sum of
// every particle's own path (smc_sum_*).  Everything per env is summed in double in
// a fixed order (no atomics), the tick counter lives on the device, and nothing is
// read back, so a tick can be captured and replayed.  The host arithmetic (sizes,
// refusal bounds, segments, variant, grids) is smc_sizes.h.
#include "planner_common.h"
#include "smc_sizes.h"

namespace {

struct SigmaArg {
  float sigma[4];
  __device__ __forceinline__ float at(size_t, int a) const { return sigma[a]; }
};

struct BeginParams {
  double* base;              // [C][E]
  int32_t* parents;          // [S][C][E]
  double* ess;               // [S][E]
  double* offset;            // [S][E]
  int32_t* resampled;        // [S][E]
  uint32_t S, C, E;
};

struct WeighParams {
  const double* ret;         // [C][E]: the branch set's
  const int32_t* first_done; // [C][E]
  double* base;              // [C][E]
  double* w;                 // [C][E]
  int32_t* parents;          // [C][E]: this segment's row (resampling only)
  double* ess;               // [E]: this segment's row
  double* offset;            // [E]: ... (resampling only)
  int32_t* resampled;        // [E]: ... (resampling only)
  int32_t* best;             // [E] (finish only)
  const uint64_t* tick;
  double lambda, penalty, ess_below;   // resample iff ess < ess_below = ess_frac · C
  uint32_t k0, k1, genv0, seg;
  int n, C, E;               // n: steps since the fork, what first_done is held against
  int fd_div;                // 1 (penalised_score's)
  int resample;              // 1: qs_smc_resample; 0: qs_smc_finish (weights, ess and best only)
};

struct TraceParams {
  const int32_t* parents;    // [S][C][E]
  int32_t* ancestors;        // [S][C][E]
  int S, C, E;
};

struct SumParams {
  const float* cand;         // [n][C][E][row]
  const double* w;           // [C][E]
  const int32_t* ancestors;  // [S][C][E]
  float* nominal;            // [n][E][row]
  float* action;             // [E][row]
  uint64_t* tick;
  int n, L, C, E, row, rowp; // rowp = the power of two >= row
};

// ---- begin ------------------------------------------------------------------------
__global__ __launch_bounds__(qs::kSmcThreads) void smc_begin_kernel(BeginParams P) {
  const uint32_t t = blockIdx.x * (uint32_t)qs::kSmcThreads + threadIdx.x;   // S · C · E < 2^31
  const uint32_t V = P.C * P.E;
  if (t >= P.S * V) return;
  P.parents[t] = (int32_t)((t % V) / P.E);
  if (t < V) P.base[t] = 0.0;
  if (t < P.S * P.E) { P.ess[t] = 0.0; P.offset[t] = 0.0; P.resampled[t] = 0; }
}

// ---- weights ----------------------------------------------------------------------
using qs::score_of;
// A particle's log weight: its penalised score since it was last resampled, over lambda.
__device__ __forceinline__ double logw_of(const WeighParams& P, size_t ce) { return (score_of(P, ce) - P.base[ce]) / P.lambda; }
// exp(logw - m), 0 for a NaN; 1 for every particle where no log weight is a number (m = -inf).
__device__ __forceinline__ double x_of(double lw, double m) {
  if (m == -INFINITY) return 1.0;
  return lw != lw ? 0.0 : exp(lw - m);
}
// The resampling offset of (tick, env, segment): 24 bits in [0, 1).
__device__ __forceinline__ double offset_of(const WeighParams& P, int e) {
  const qs::U4 x = qs::philox(qs::U4{(uint32_t)*P.tick, P.genv0 + (uint32_t)e, P.seg, (uint32_t)qs::kSmcOffsetTag << 24}, P.k0, P.k1);
  return (double)(x.x >> 8) * (1.0 / 16777216.0);
}

// One thread per env.  The cumulative weight is the running sum in index order; the
// C positions (i + u) / C rise with i, so one walk along it finds every parent.
__global__ __launch_bounds__(qs::kSmcThreads) void smc_weigh_thread_kernel(WeighParams P) {
  const int e = blockIdx.x * qs::kSmcThreads + threadIdx.x;
  if (e >= P.E) return;
  double m = -INFINITY;
  for (int c = 0; c < P.C; ++c) {
    const double lw = logw_of(P, (size_t)c * P.E + e);
    if (lw > m) m = lw;   // (false for a NaN)
  }
  double sum = 0.0;
  for (int c = 0; c < P.C; ++c) {
    const size_t ce = (size_t)c * P.E + e;
    const double x = x_of(logw_of(P, ce), m);
    P.w[ce] = x;
    sum += x;
  }
  double sq = 0.0, wb = -1.0;
  int cb = 0;
  for (int c = 0; c < P.C; ++c) {
    const size_t ce = (size_t)c * P.E + e;
    const double w = P.w[ce] / sum;
    P.w[ce] = w;
    sq += w * w;
    if (w > wb) { wb = w; cb = c; }
  }
  const double ess = 1.0 / sq;
  P.ess[e] = ess;
  if (!P.resample) {
    P.best[e] = cb;
    return;
  }
  const bool go = m != -INFINITY && ess < P.ess_below;
  P.resampled[e] = go ? 1 : 0;
  if (!go) {
    P.offset[e] = 0.0;
    for (int c = 0; c < P.C; ++c) P.parents[(size_t)c * P.E + e] = c;
    return;
  }
  const double u = offset_of(P, e);
  P.offset[e] = u;
  int c = 0;
  double cum = P.w[e];
  for (int i = 0; i < P.C; ++i) {
    const double pos = ((double)i + u) / (double)P.C;
    while (!(cum > pos) && c < P.C - 1) {
      ++c;
      cum += P.w[(size_t)c * P.E + e];
    }
    P.parents[(size_t)i * P.E + e] = c;
    // the new particle i starts at log weight 0.  base is not read again in this
    // launch (the log weights above were the last), so rows below c may be overwritten.
    P.base[(size_t)i * P.E + e] = score_of(P, (size_t)c * P.E + e);
  }
}

// An inclusive and an exclusive scan over the workgroup's threads in thread order:
// Hillis-Steele inside a wave, then the waves before this one folded in order
// (sh holds one double a wave).  Ends in a barrier, after which sh may be reused.
template <class Op>
__device__ __forceinline__ void block_scan(double v, double identity, Op op, double* sh, int tid, double* incl, double* excl) {
  constexpr int kWaves = qs::kSmcBlockThreads / 64;
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double up = __shfl_up(v, off, 64);
    if (lane >= off) v = op(up, v);
  }
  double before = __shfl_up(v, 1, 64);
  if (lane == 0) before = identity;
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  double pre = identity;
  for (int k = 0; k < kWaves; ++k)
    if (k < wave) pre = op(pre, sh[k]);
  __syncthreads();
  *incl = op(pre, v);
  *excl = op(pre, before);
}
struct AddOp { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };
struct MaxOp { __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; } };

// block_row_reduce's sum of one value a thread, handed to every thread.
__device__ __forceinline__ double block_sum(double acc, double* part, int tid) {
  qs::block_row_reduce(acc, part, tid, 1);
  const double total = part[0];
  __syncthreads();   // part is used again
  return total;
}

// One workgroup per env: thread t holds the K = ceil(C / 1024) <= kSmcScanPerThread
// particles t · K .. t · K + K - 1, so the cumulative weight is a scan over the
// threads in order.  Two scans: the sum, then a running maximum over it, because
// partial sums that the scan forms along different trees need not rise with c in
// floating point, and the binary search below (and the order of the parents) needs
// that.  The cumulative weights stay in LDS, one double a particle.
__global__ __launch_bounds__(qs::kSmcBlockThreads) void smc_weigh_block_kernel(WeighParams P) {
  constexpr int kThreads = qs::kSmcBlockThreads, kWaves = kThreads / 64, kPer = qs::kSmcScanPerThread;
  __shared__ double sh_cum[qs::kSmcMaxParticles];
  __shared__ double sh_part[kWaves];
  __shared__ int sh_c[kWaves];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = (P.C + kThreads - 1) / kThreads, c0 = tid * K;
  double lw[kPer], w[kPer];
  double m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int c = c0 + k;
    const bool have = k < K && c < P.C;
    lw[k] = have ? logw_of(P, (size_t)c * P.E + e) : NAN;
    if (lw[k] > m) m = lw[k];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double m2 = __shfl_xor(m, off, 64);
    if (m2 > m) m = m2;
  }
  if (lane == 0) sh_part[wave] = m;
  __syncthreads();
  m = sh_part[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) m = sh_part[k] > m ? sh_part[k] : m;
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    w[k] = (k < K && c0 + k < P.C) ? x_of(lw[k], m) : 0.0;
    acc += w[k];
  }
  const double sum = block_sum(acc, sh_part, tid);
  double sq = 0.0, wb = -1.0;
  int cb = INT32_MAX;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int c = c0 + k;
    if (k < K && c < P.C) {
      w[k] /= sum;
      P.w[(size_t)c * P.E + e] = w[k];
      sq += w[k] * w[k];
      if (w[k] > wb) { wb = w[k]; cb = c; }
    }
  }
  const double ess = 1.0 / block_sum(sq, sh_part, tid);
  if (tid == 0) P.ess[e] = ess;
  if (!P.resample) {   // finish: the lowest c of the largest weight
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double w2 = __shfl_xor(wb, off, 64);
      const int c2 = __shfl_xor(cb, off, 64);
      if (w2 > wb || (w2 == wb && c2 < cb)) { wb = w2; cb = c2; }
    }
    if (lane == 0) { sh_part[wave] = wb; sh_c[wave] = cb; }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < kWaves; ++k)
        if (sh_part[k] > wb || (sh_part[k] == wb && sh_c[k] < cb)) { wb = sh_part[k]; cb = sh_c[k]; }
      P.best[e] = cb < P.C ? cb : 0;   // (every weight a NaN: no comparison held)
    }
    return;
  }
  const bool go = m != -INFINITY && ess < P.ess_below;   // (the same for every thread: m and ess came through LDS)
  if (tid == 0) P.resampled[e] = go ? 1 : 0;
  if (!go) {
    if (tid == 0) P.offset[e] = 0.0;
    for (int c = tid; c < P.C; c += kThreads) P.parents[(size_t)c * P.E + e] = c;
    return;
  }
  const double u = offset_of(P, e);
  if (tid == 0) P.offset[e] = u;
  double mine = 0.0, incl, before;
#pragma unroll
  for (int k = 0; k < kPer; ++k) mine += w[k];   // (0 beyond the thread's particles)
  block_scan(mine, 0.0, AddOp(), sh_part, tid, &incl, &before);
  double cum[kPer], run = 0.0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    run += w[k];
    cum[k] = before + run;   // rises with k: w >= 0
  }
  double floor_incl, floor_before;
  block_scan(cum[kPer - 1], 0.0, MaxOp(), sh_part, tid, &floor_incl, &floor_before);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int c = c0 + k;
    if (k < K && c < P.C) sh_cum[c] = cum[k] > floor_before ? cum[k] : floor_before;
  }
  __syncthreads();
  for (int i = tid; i < P.C; i += kThreads) {
    const double pos = ((double)i + u) / (double)P.C;
    int lo = 0, hi = P.C - 1;   // the lowest c in lo .. hi with sh_cum[c] > pos, or C - 1
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sh_cum[mid] > pos) hi = mid;
      else lo = mid + 1;
    }
    P.parents[(size_t)i * P.E + e] = lo;
    // base was last read for the log weights, barriers ago
    P.base[(size_t)i * P.E + e] = score_of(P, (size_t)lo * P.E + e);
  }
}

// ---- ancestry: one thread per (c, e) walks the segments down ------------------------
__global__ __launch_bounds__(qs::kSmcThreads) void smc_trace_kernel(TraceParams P) {
  const uint32_t t = blockIdx.x * (uint32_t)qs::kSmcThreads + threadIdx.x;
  const uint32_t V = (uint32_t)P.C * (uint32_t)P.E;
  if (t >= V) return;
  const uint32_t e = t % (uint32_t)P.E;
  int a = (int)(t / (uint32_t)P.E);
  for (int s = P.S - 1; s >= 0; --s) {
    P.ancestors[(size_t)s * V + t] = a;
    if (s > 0) {
      a = P.parents[(size_t)(s - 1) * V + (size_t)a * P.E + e];
      a = a < 0 ? 0 : (a >= P.C ? P.C - 1 : a);   // (the kernels write 0 .. C - 1; a caller's bytes stay in range too)
    }
  }
}

// ---- weighted sum of the particles' own paths ---------------------------------------
// new[j][e][k] goes where the shifted nominal wants it (nothing here reads the nominal).
__device__ __forceinline__ void store_new(const SumParams& P, int j, int e, int k, float v) {
  const size_t ek = (size_t)e * P.row + k, step = (size_t)P.E * P.row;
  if (j == 0) P.action[ek] = v;
  else P.nominal[(size_t)(j - 1) * step + ek] = v;
  if (j == P.n - 1) P.nominal[(size_t)j * step + ek] = v;   // hold
}

// One thread per (j, e, d, a).
__global__ __launch_bounds__(qs::kSmcThreads) void smc_sum_thread_kernel(SumParams P) {
  const uint64_t t = (uint64_t)blockIdx.x * qs::kSmcThreads + threadIdx.x;
  if (t == 0) *P.tick += 1;
  const size_t step = (size_t)P.E * P.row;
  if (t >= (uint64_t)P.n * step) return;
  const int j = (int)(t / step);
  const size_t ek = t % step;
  const int e = (int)(ek / P.row), k = (int)(ek % P.row);
  const float* cj = P.cand + (size_t)j * P.C * step + ek;
  const int32_t* anc = P.ancestors + (size_t)(j / P.L) * P.C * P.E + e;
  double acc = 0.0;
  for (int c = 0; c < P.C; ++c) acc += P.w[(size_t)c * P.E + e] * (double)cj[(size_t)anc[(size_t)c * P.E] * step];
  store_new(P, j, e, k, (float)acc);
}

// One workgroup per (env, step): thread t holds component k = t mod rowp of particle
// group g = t / rowp and strides over c by the group count; block_row_reduce sums the groups.
__global__ __launch_bounds__(qs::kSmcBlockThreads) void smc_sum_block_kernel(SumParams P) {
  __shared__ double part[qs::kSmcBlockThreads];
  const int e = blockIdx.x % P.E, j = blockIdx.x / P.E;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) *P.tick += 1;
  const int rowp = P.rowp, k = tid & (rowp - 1), g = tid / rowp, G = qs::kSmcBlockThreads / rowp;
  const size_t step = (size_t)P.E * P.row;
  const float* cj = P.cand + (size_t)j * P.C * step + (size_t)e * P.row;
  const int32_t* anc = P.ancestors + (size_t)(j / P.L) * P.C * P.E + e;
  double acc = 0.0;
  if (k < P.row) {
#pragma unroll 4
    for (int c = g; c < P.C; c += G) acc += P.w[(size_t)c * P.E + e] * (double)cj[(size_t)anc[(size_t)c * P.E] * step + k];
  }
  qs::block_row_reduce(acc, part, tid, rowp);
  if (tid < P.row) store_new(P, j, e, tid, (float)part[tid]);
}

}  // namespace

struct qs_smc : qs::PlannerBase {
  qs_smc_spec spec;
  int L, S;
  qs::SmcVariant variant;
  qs::SmcGrids grids;
  uint64_t bytes[qs::kSmcBufs];
  void* buf[qs::kSmcBufs];
  qs_branch* set = nullptr;
  qs_branch_bufs set_bufs{};
  bool begun = false;      // qs_smc_begin has forked the set
};

namespace {

int begin_impl(qs_smc* p, void* stream) {
  if (int rc = qs_branch_fork(p->set, stream)) return rc;
  p->begun = true;
  BeginParams P;
  P.base = (double*)p->buf[qs::kSmcBase];
  P.parents = (int32_t*)p->buf[qs::kSmcParents];
  P.ess = (double*)p->buf[qs::kSmcEss];
  P.offset = (double*)p->buf[qs::kSmcOffset];
  P.resampled = (int32_t*)p->buf[qs::kSmcResampled];
  P.S = (uint32_t)p->S; P.C = (uint32_t)p->C; P.E = (uint32_t)p->E;
  hipLaunchKernelGGL(smc_begin_kernel, dim3(p->grids.begin), dim3(qs::kSmcThreads), 0, (hipStream_t)stream, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

// The shared sample kernel over the steps of segment s: tag 5, the segment where CEM has its iteration.
int sample_impl(qs_smc* p, int s, hipStream_t st) {
  const size_t col = (size_t)p->E * p->D * p->A, start = (size_t)qs::smc_segment_start(p->L, s);
  const int len = (int)qs::smc_segment_length(p->n, p->L, s);
  qs::SampleParams<SigmaArg> P;
  P.mean = (const float*)p->buf[qs::kSmcNominal] + start * col;
  P.cand = (float*)p->buf[qs::kSmcCandidates] + start * (size_t)p->C * col;
  P.tick = (const uint64_t*)p->buf[qs::kSmcTick];
  P.k0 = (uint32_t)p->spec.seed; P.k1 = (uint32_t)(p->spec.seed >> 32);
  P.genv0 = (uint32_t)p->info.env_offset;
  P.tag = (uint32_t)qs::kSmcTag; P.iter = (uint32_t)s;
  P.n = len; P.C = p->C; P.E = p->E; P.D = p->D; P.A = p->A;
  for (int a = 0; a < 4; ++a) P.spread.sigma[a] = p->spec.sigma[a];
  P.lo = p->spec.lo; P.hi = p->spec.hi;
  // with a correlated sampling spec (qs_sampling_smc_set) the recurrence runs over these `len` steps only: it
  // restarts at every segment, since resampling reassigns the particles in between
  return qs::planner_launch_sample(p, P, p->grids.sample, st);
}

int advance_impl(qs_smc* p, int s, void* stream) {
  const int len = (int)qs::smc_segment_length(p->n, p->L, s);
  return qs_branch_advance(p->set, len, p->steps.data() + qs::smc_segment_start(p->L, s), nullptr, stream);
}

// The weights of the particles `steps` steps after the fork into row s of ess; resample: and parents[s], base.
int weigh_impl(qs_smc* p, int s, int steps, bool resample, hipStream_t st) {
  WeighParams P;
  P.ret = p->set_bufs.ret;
  P.first_done = p->set_bufs.first_done;
  P.base = (double*)p->buf[qs::kSmcBase];
  P.w = (double*)p->buf[qs::kSmcWeights];
  P.parents = (int32_t*)p->buf[qs::kSmcParents] + (size_t)s * p->C * p->E;
  P.ess = (double*)p->buf[qs::kSmcEss] + (size_t)s * p->E;
  P.offset = (double*)p->buf[qs::kSmcOffset] + (size_t)s * p->E;
  P.resampled = (int32_t*)p->buf[qs::kSmcResampled] + (size_t)s * p->E;
  P.best = (int32_t*)p->buf[qs::kSmcBest];
  P.tick = (const uint64_t*)p->buf[qs::kSmcTick];
  P.lambda = p->spec.lambda;
  P.penalty = p->spec.done_penalty;
  P.ess_below = p->spec.ess_frac * (double)p->C;
  P.k0 = (uint32_t)p->spec.seed; P.k1 = (uint32_t)(p->spec.seed >> 32);
  P.genv0 = (uint32_t)p->info.env_offset;
  P.seg = (uint32_t)s;
  P.n = steps; P.C = p->C; P.E = p->E;
  P.fd_div = 1;
  P.resample = resample ? 1 : 0;
  if (p->variant == qs::kSmcPerBlock)
    hipLaunchKernelGGL(smc_weigh_block_kernel, dim3(p->grids.weigh), dim3(qs::kSmcBlockThreads), 0, st, P);
  else
    hipLaunchKernelGGL(smc_weigh_thread_kernel, dim3(p->grids.weigh), dim3(qs::kSmcThreads), 0, st, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

// Nothing for the last segment (finish weighs it) or with ess_frac = 0.
int resample_impl(qs_smc* p, int s, void* stream) {
  if (s == p->S - 1 || p->spec.ess_frac == 0.0) return QS_OK;
  if (int rc = weigh_impl(p, s, (s + 1) * p->L, true, (hipStream_t)stream)) return rc;
  return qs_branch_select(p->set, (const int32_t*)p->buf[qs::kSmcParents] + (size_t)s * p->C * p->E, stream);
}

int finish_impl(qs_smc* p, hipStream_t st) {
  if (int rc = weigh_impl(p, p->S - 1, p->n, false, st)) return rc;
  TraceParams T;
  T.parents = (const int32_t*)p->buf[qs::kSmcParents];
  T.ancestors = (int32_t*)p->buf[qs::kSmcAncestors];
  T.S = p->S; T.C = p->C; T.E = p->E;
  hipLaunchKernelGGL(smc_trace_kernel, dim3(p->grids.trace), dim3(qs::kSmcThreads), 0, st, T);
  PLANNER_HIP_TRY(hipGetLastError());
  SumParams P;
  P.cand = (const float*)p->buf[qs::kSmcCandidates];
  P.w = (const double*)p->buf[qs::kSmcWeights];
  P.ancestors = (const int32_t*)p->buf[qs::kSmcAncestors];
  P.nominal = (float*)p->buf[qs::kSmcNominal];
  P.action = (float*)p->buf[qs::kSmcAction];
  P.tick = (uint64_t*)p->buf[qs::kSmcTick];
  P.n = p->n; P.L = p->L; P.C = p->C; P.E = p->E;
  P.row = p->row();
  P.rowp = qs::mppi_row_pow2(P.row);
  if (p->variant == qs::kSmcPerBlock)
    hipLaunchKernelGGL(smc_sum_block_kernel, dim3(p->grids.sum), dim3(qs::kSmcBlockThreads), 0, st, P);
  else
    hipLaunchKernelGGL(smc_sum_thread_kernel, dim3(p->grids.sum), dim3(qs::kSmcThreads), 0, st, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

// QS_OK, or the refusal of a segment index outside 0 .. S - 1.
int check_segment(const qs_smc* p, int s, const char* who) {
  if (qs::smc_segment_index_ok(p->n, p->L, s)) return QS_OK;
  return qs::set_last_error(QS_E_INVALID, std::string(who) + ": segment = " + std::to_string(s) +
                                              " is outside 0 .. segments - 1 = " + std::to_string(p->S - 1));
}

int not_begun(const char* who) {
  return qs::set_last_error(QS_E_STATE, std::string(who) + ": call qs_smc_begin first");
}

}  // namespace

extern "C" {

int qs_smc_create(qs_handle* h, const qs_smc_spec* spec, qs_smc** out) {
  const char* who = "qs_smc_create";
  const std::string w = std::string(who) + ": ";
  using qs::set_last_error;
  if (!h || !spec || !out) return set_last_error(QS_E_INVALID, w + "null argument");
  const int depth = qs_score_depth(h);
  if (depth < 1)
    return set_last_error(QS_E_INVALID, w + "this handle cannot score (qs_score_depth = 0): a layout whose "
                                            "reset draws can be rejected, or a Flock / Meetup / LeaderFollower task");
  if (!qs::smc_segment_ok(spec->segment, depth))
    return set_last_error(QS_E_INVALID, w + "segment = " + std::to_string(spec->segment) +
                                            " is outside 1 .. qs_score_depth = " + std::to_string(depth));
  if (spec->horizon < 1 || (int64_t)spec->horizon > (int64_t)qs::kSmcMaxSegments * spec->segment)
    return set_last_error(QS_E_INVALID, w + "horizon = " + std::to_string(spec->horizon) + " is outside 1 .. " +
                                            std::to_string(qs::kSmcMaxSegments) + " segments of " + std::to_string(spec->segment));
  if (spec->particles < 2 || spec->particles > qs::kSmcMaxParticles)
    return set_last_error(QS_E_INVALID, w + "particles = " + std::to_string(spec->particles) + " is outside 2 .. " +
                                            std::to_string(qs::kSmcMaxParticles) + " (particle 0 follows the nominal)");
  if (!qs::smc_clip_ok(spec->lo, spec->hi)) return set_last_error(QS_E_INVALID, w + "lo must be below hi, both finite");
  qs_dims d;
  if (int rc = qs_get_dims(h, &d)) return rc;
  for (int a = 0; a < d.act_dim && a < 4; ++a)
    if (!qs::smc_sigma_ok(spec->sigma[a]))
      return set_last_error(QS_E_INVALID, w + "sigma[" + std::to_string(a) + "] must be finite and >= 0");
  if (!qs::smc_penalty_ok(spec->done_penalty)) return set_last_error(QS_E_INVALID, w + "done_penalty must be finite and >= 0");
  if (!qs::smc_lambda_ok(spec->lambda)) return set_last_error(QS_E_INVALID, w + "lambda must be finite and > 0");
  if (!qs::smc_ess_frac_ok(spec->ess_frac)) return set_last_error(QS_E_INVALID, w + "ess_frac must be in [0, 1]");
  const qs::SmcShape shape{spec->horizon, spec->segment, spec->particles, d.num_envs, d.num_drones, d.act_dim};
  uint64_t bytes[qs::kSmcBufs];
  const qs::SmcVariant variant = qs::smc_variant(shape.E, shape.C, shape.D * shape.A);
  if (!qs::smc_sizes(shape, bytes) || !qs::smc_grids_fit(shape, variant))
    return set_last_error(QS_E_INVALID, w + "particles * num_envs * num_drones (or the [segments][particles][num_envs] "
                                            "tables) is too large (32-bit offsets)");
  qs_branch* set = nullptr;
  if (int rc = qs_branch_create(h, spec->particles, &set)) return rc;   // (its own refusals and message)
  qs_smc* p = new (std::nothrow) qs_smc;
  if (!p) {
    qs_branch_destroy(set);
    return set_last_error(QS_E_NOMEM, w + "out of host memory");
  }
  p->h = h;
  p->spec = *spec;
  qs::handle_info(h, &p->info);
  p->n = spec->horizon; p->C = spec->particles; p->E = d.num_envs; p->D = d.num_drones; p->A = d.act_dim;
  p->L = spec->segment;
  p->S = (int)qs::smc_segments(p->n, p->L);
  p->variant = variant;
  p->grids = qs::smc_grids(shape, variant);
  for (int i = 0; i < qs::kSmcBufs; ++i) { p->bytes[i] = bytes[i]; p->buf[i] = nullptr; }
  if (int rc = qs::planner_alloc(who, p, qs::kSmcCandidates)) {   // (deletes p on failure)
    qs_branch_destroy(set);
    return rc;
  }
  p->set = set;
  (void)qs_branch_buffers(set, &p->set_bufs);
  *out = p;
  return QS_OK;
}

int qs_smc_destroy(qs_smc* p) {
  if (!p) return QS_OK;
  qs_branch_destroy(p->set);
  return qs::planner_destroy(p);
}

int qs_smc_buffers(const qs_smc* p, qs_smc_bufs* out) {
  if (!p || !out) return qs::set_last_error(QS_E_INVALID, "qs_smc_buffers: null argument");
  out->nominal = (float*)p->buf[qs::kSmcNominal];
  out->candidates = (float*)p->buf[qs::kSmcCandidates];
  out->base = (double*)p->buf[qs::kSmcBase];
  out->weights = (double*)p->buf[qs::kSmcWeights];
  out->parents = (int32_t*)p->buf[qs::kSmcParents];
  out->ancestors = (int32_t*)p->buf[qs::kSmcAncestors];
  out->ess = (double*)p->buf[qs::kSmcEss];
  out->offset = (double*)p->buf[qs::kSmcOffset];
  out->resampled = (int32_t*)p->buf[qs::kSmcResampled];
  out->best = (int32_t*)p->buf[qs::kSmcBest];
  out->action = (float*)p->buf[qs::kSmcAction];
  out->tick = (uint64_t*)p->buf[qs::kSmcTick];
  return QS_OK;
}

int qs_smc_branch(const qs_smc* p, qs_branch** out) {
  if (!p || !out) return qs::set_last_error(QS_E_INVALID, "qs_smc_branch: null argument");
  *out = p->set;
  return QS_OK;
}

int qs_smc_reset(qs_smc* p, const float* nominal, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_reset: null planner");
  return qs::planner_reset(p, qs::kSmcNominal, qs::kSmcTick, nominal, (hipStream_t)stream);
}

int qs_smc_begin(qs_smc* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_begin: null planner");
  if (int rc = qs::planner_ready("qs_smc_begin", p)) return rc;
  return begin_impl(p, stream);
}

int qs_smc_sample(qs_smc* p, int segment, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_sample: null planner");
  if (int rc = check_segment(p, segment, "qs_smc_sample")) return rc;
  return sample_impl(p, segment, (hipStream_t)stream);
}

int qs_smc_advance(qs_smc* p, int segment, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_advance: null planner");
  if (int rc = check_segment(p, segment, "qs_smc_advance")) return rc;
  if (!p->begun) return not_begun("qs_smc_advance");
  return advance_impl(p, segment, stream);
}

int qs_smc_resample(qs_smc* p, int segment, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_resample: null planner");
  if (int rc = check_segment(p, segment, "qs_smc_resample")) return rc;
  if (!p->begun) return not_begun("qs_smc_resample");
  return resample_impl(p, segment, stream);
}

int qs_smc_finish(qs_smc* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_finish: null planner");
  return finish_impl(p, (hipStream_t)stream);
}

int qs_sampling_smc_set(qs_smc* p, const qs_sampling_spec* spec) {
  return qs::sampling_attach("qs_sampling_smc_set", p, qs::kSamplingSmc, 0, spec);
}

int qs_smc_plan(qs_smc* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_smc_plan: null planner");
  if (int rc = qs::planner_ready("qs_smc_plan", p)) return rc;
  if (int rc = begin_impl(p, stream)) return rc;
  for (int s = 0; s < p->S; ++s) {
    if (int rc = sample_impl(p, s, (hipStream_t)stream)) return rc;
    if (int rc = advance_impl(p, s, stream)) return rc;
    if (int rc = resample_impl(p, s, stream)) return rc;
  }
  return finish_impl(p, (hipStream_t)stream);
}

}  // extern "C"
