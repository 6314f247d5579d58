// planner_cem.hip — the CEM planner tick on top of qs_score (include/quadswarm.h,
// qs_cem_*; DESIGN.md §4a "CEM tick").
//
// A tick is begin, I × (sample, qs_score, refit), finish (with a policy prior
// attached, planner_prior.hip: begin, the prior stage, and every sample followed by
// the inject launch).  With a sampling spec (qs_sampling_cem_set, sampling_sizes.h) a
// non-zero rho swaps the sample launch for planner_sample_ar_kernel, one launch for
// one, and keep > 0 adds the elite memory inside the launches there are: the refit
// kernel also stores the first `keep` elite rows it reads into `kept`, the sample
// kernel copies them over candidates 1 .. *kept_n in place of drawing those, and the
// finish kernel's grid grows by kept's columns, which it shifts as it shifts the mean.
// The launch count of a tick is the same with and without the spec.
// The sample is
// planner_sample_kernel (shared with the MPPI tick, planner_common.h) with a
// per-element spread and the iteration in the Philox counter; cem_select_* ranks
// an env's candidates by their penalised
// score and writes the K best in rank order; cem_refit_* fits a mean and a
// standard deviation per (step, drone, component) to those K rows.  Everything
// per env is summed in double in a fixed order (no float atomics; the select's
// histogram uses integer LDS atomics, whose sums do not depend on their order),
// the tick counter lives on the device, and nothing is read back, so a tick can
// be captured and replayed.  The host arithmetic (sizes, variant, grids) is
// cem_sizes.h.
#include "planner_common.h"
#include "cem_sizes.h"

namespace {

// The spread of an element, from memory.
struct StdMem {
  const float* std;          // [n][E][D][A]
  __device__ __forceinline__ float at(size_t i, int a) const { return std[i + a]; }
};

// In the select and refit records E counts the units that are ranked on their own
// and row their components: the envs and D · A, or in per-drone mode the E · D
// agents and A (planner_common.h, PlannerBase).  Either way [E][row] is [envs][D][A].
struct SelectParams {
  const double* ret;         // [C][E]: ret, or in per-drone mode ret_agent
  const int32_t* first_done; // [C][E / fd_div]
  int32_t* elites;           // [K][E]
  double* iter_best;         // [E]: this iteration's row
  double penalty;
  int n, C, K, E;
  int index_bytes;           // cem_index_bytes(C)
  int fd_div;                // 1, or in per-drone mode D
};

struct RefitParams {
  const float* cand;         // [n][C][E][row]
  const int32_t* elites;     // [K][E]
  float* mean;               // [n][E][row]
  float* std;                // [n][E][row]
  double alpha;
  int n, C, K, E, A, row, rowp;   // rowp = the power of two >= row
  float sigma[4], sigma_min[4];
  // The elite memory (a sampling spec with keep > 0; null: none): the refit also
  // writes kept[j][r][e][row] = cand[j][elites[r][e]][e][row] for r < keep, the values
  // it reads anyway, and *kept_n = keep.  In per-drone mode e is an agent, so a kept
  // row is the composite of every drone's own r-th elite slice.
  float* kept;               // [n][keep][E][row]
  int32_t* kept_n;           // [1]
  int keep;
};

struct FillParams {
  float* std;                // [n][E][D][A]
  uint64_t total;            // n · E · D · A
  int A;
  float sigma[4];
};

struct FinishParams {
  float* mean;               // [n][E][D][A]
  float* action;             // [E][D][A]
  uint64_t* tick;
  uint64_t col;              // E · D · A
  int n;
  float* kept;               // [n][keep][E][D][A], or null: the elite memory shifts as the mean does
  uint64_t kept_col;         // keep · E · D · A
};

// ---- begin: the spread restarts at sigma ---------------------------------------
__global__ __launch_bounds__(qs::kCemThreads) void cem_fill_kernel(FillParams P) {
  const uint64_t t = (uint64_t)blockIdx.x * qs::kCemThreads + threadIdx.x;
  if (t >= P.total) return;
  P.std[t] = P.sigma[(int)(t % (uint64_t)P.A)];
}

// ---- the order --------------------------------------------------------------------
using qs::score_of;
// A score as an unsigned key that sorts as the total order wants: larger score,
// larger key; -0.0 and 0.0 share one key; every NaN gets 0, below -inf's key.
__device__ __forceinline__ uint64_t key_of(double s) {
  if (s != s) return 0;
  if (s == 0.0) s = 0.0;   // -0.0 -> 0.0
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// Whether (k2, c2) comes before (k1, c1): the larger key, the lower c on a tie.
__device__ __forceinline__ bool comes_before(uint64_t k2, int c2, uint64_t k1, int c1) {
  return k2 > k1 || (k2 == k1 && c2 < c1);
}

// ---- select, one thread per env ------------------------------------------------
// A candidate's rank is the number of candidates that come before it; the order
// is total, so the ranks are 0 .. C - 1, each once.
__global__ __launch_bounds__(qs::kCemThreads) void cem_select_thread_kernel(SelectParams P) {
  const int e = blockIdx.x * qs::kCemThreads + threadIdx.x;
  if (e >= P.E) return;
  for (int c = 0; c < P.C; ++c) {
    const double s = score_of(P, (size_t)c * P.E + e);
    const uint64_t k = key_of(s);
    int rank = 0;
    for (int c2 = 0; c2 < P.C; ++c2) rank += comes_before(key_of(score_of(P, (size_t)c2 * P.E + e)), c2, k, c) ? 1 : 0;
    if (rank < P.K) P.elites[(size_t)rank * P.E + e] = c;
    if (rank == 0) P.iter_best[e] = s;
  }
}

// ---- select, one workgroup per env -------------------------------------------------
// The (key, C - 1 - c) pairs are distinct, so exactly K of them are >= the K-th
// largest.  That pair is found a byte at a time from the top (8 passes over the
// key, index_bytes over the index): a 256-bin histogram of the byte among the
// candidates that match the bytes fixed so far, then wave 0 walks it from 255
// down to the bin where the running count reaches what is still wanted.  The
// passes end early once that bin holds exactly what is still wanted: whatever
// matches the bytes fixed so far is then at or above the threshold.  The K
// candidates at or above the threshold are gathered in LDS (in arrival order) and
// ranked among themselves by counting, which puts them in the total order.
__global__ __launch_bounds__(qs::kCemBlockThreads) void cem_select_block_kernel(SelectParams P) {
  constexpr int kThreads = qs::kCemBlockThreads;
  __shared__ uint64_t sh_key[qs::kCemStage];
  __shared__ uint64_t sh_ek[qs::kCemMaxElites];
  __shared__ int32_t sh_ec[qs::kCemMaxElites];
  __shared__ uint32_t sh_hist[256];
  __shared__ uint32_t sh_digit, sh_want, sh_done, sh_count;
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int staged = P.C < qs::kCemStage ? P.C : qs::kCemStage;
  for (int c = tid; c < staged; c += kThreads) sh_key[c] = key_of(score_of(P, (size_t)c * P.E + e));
  if (tid == 0) sh_count = 0;
  sh_ek[tid] = 0;   // (kCemMaxElites = kThreads slots; exactly K are filled below)
  sh_ec[tid] = 0;
  __syncthreads();
  auto key_at = [&](int c) -> uint64_t { return c < staged ? sh_key[c] : key_of(score_of(P, (size_t)c * P.E + e)); };

  uint64_t key_mask = 0, key_fix = 0;   // the bytes fixed so far, and their values
  uint32_t idx_mask = 0, idx_fix = 0;
  uint32_t want = (uint32_t)P.K;        // the threshold is the want-th largest among the matching
  const int passes = 8 + P.index_bytes;
  for (int pass = 0; pass < passes; ++pass) {
    const bool in_key = pass < 8;
    const int shift = in_key ? 56 - 8 * pass : 8 * (P.index_bytes - 1 - (pass - 8));
    if (tid < 256) sh_hist[tid] = 0;
    __syncthreads();
    for (int base = 0; base < P.C; base += kThreads) {   // (a whole wave takes every trip: the ballots below)
      const int c = base + tid;
      bool active = false;
      uint32_t digit = 0;
      if (c < P.C) {
        const uint64_t k = key_at(c);
        const uint32_t ix = (uint32_t)(P.C - 1 - c);
        if ((k & key_mask) == key_fix && (ix & idx_mask) == idx_fix) {
          active = true;
          digit = in_key ? (uint32_t)(k >> shift) & 255u : (ix >> shift) & 255u;
        }
      }
      // scores of one magnitude share their top bytes: one add a wave where every lane names the same bin
      const unsigned long long act = __ballot(active);
      if (act != 0) {
        const int first = __ffsll((long long)act) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)digit, first, 64);
        const unsigned long long same = __ballot(active && digit == d0);
        if (same == act) {
          if (lane == first) atomicAdd(&sh_hist[d0], (uint32_t)__popcll(act));
        } else if (active) {
          atomicAdd(&sh_hist[digit], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < 64) {   // wave 0: lane l holds bins 255 - 4l .. 252 - 4l, from the top
      uint32_t h[4], own = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { h[q] = sh_hist[255 - 4 * lane - q]; own += h[q]; }
      uint32_t incl = own;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += up;
      }
      uint32_t run = incl - own;
      if (run < want && want <= incl) {   // one lane: the matching candidates are at least `want`
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (run < want && want <= run + h[q]) {
            sh_digit = (uint32_t)(255 - 4 * lane - q);
            sh_want = want - run;
            sh_done = h[q] == want - run ? 1u : 0u;   // every candidate left in the bin is wanted
          }
          run += h[q];
        }
      }
    }
    __syncthreads();
    const uint32_t g = sh_digit;
    want = sh_want;
    if (in_key) { key_mask |= 255ull << shift; key_fix |= (uint64_t)g << shift; }
    else { idx_mask |= 255u << shift; idx_fix |= g << shift; }
    if (sh_done) break;   // (the same word for every thread; written again two barriers on)
  }
  // the threshold pair, as far as its bytes were needed, is (key_fix, idx_fix): gather what is at or above it
  for (int c = tid; c < P.C; c += kThreads) {
    const uint64_t k = key_at(c), km = k & key_mask;
    const uint32_t im = (uint32_t)(P.C - 1 - c) & idx_mask;
    if (km > key_fix || (km == key_fix && im >= idx_fix)) {
      const uint32_t slot = atomicAdd(&sh_count, 1u);
      if (slot < (uint32_t)qs::kCemMaxElites) { sh_ek[slot] = k; sh_ec[slot] = c; }
    }
  }
  __syncthreads();
  if (tid < P.K) {
    const uint64_t k = sh_ek[tid];
    const int c = sh_ec[tid];
    int rank = 0;
#pragma unroll 8
    for (int m = 0; m < P.K; ++m) rank += comes_before(sh_ek[m], sh_ec[m], k, c) ? 1 : 0;   // broadcast reads
    P.elites[(size_t)rank * P.E + e] = c;
    if (rank == 0) P.iter_best[e] = score_of(P, (size_t)c * P.E + e);
  }
}

// ---- refit ------------------------------------------------------------------------
__device__ __forceinline__ void store_fit(const RefitParams& P, int j, int e, int k, double m, double v) {
  const size_t at = ((size_t)j * P.E + e) * P.row + k;
  const int a = k % P.A;
  float mu, sd;
  if (P.alpha == 0.0) {   // the old values are not read
    mu = (float)m;
    sd = (float)sqrt(v);
  } else {
    mu = (float)((1.0 - P.alpha) * m + P.alpha * (double)P.mean[at]);
    sd = (float)((1.0 - P.alpha) * sqrt(v) + P.alpha * (double)P.std[at]);
  }
  P.mean[at] = mu;
  if (P.sigma[a] != 0.0f) P.std[at] = fmaxf(sd, P.sigma_min[a]);
}

// One thread per (j, e, d, a), looping over the K elites in rank order; the
// threads of one env's row read one candidate row together.
__global__ __launch_bounds__(qs::kCemThreads) void cem_refit_thread_kernel(RefitParams P) {
  const uint64_t t = (uint64_t)blockIdx.x * qs::kCemThreads + threadIdx.x;
  const size_t step = (size_t)P.E * P.row;
  if (t >= (uint64_t)P.n * step) return;
  const int j = (int)(t / step);
  const size_t ek = t % step;
  const int e = (int)(ek / P.row), k = (int)(ek % P.row);
  const float* cj = P.cand + (size_t)j * P.C * step + ek;
  if (t == 0 && P.kept) *P.kept_n = P.keep;
  double sum = 0.0;
  for (int r = 0; r < P.K; ++r) {
    const float x = cj[(size_t)P.elites[(size_t)r * P.E + e] * step];
    if (r < P.keep) P.kept[((size_t)j * P.keep + r) * step + ek] = x;   // (keep = 0 without elite memory)
    sum += (double)x;
  }
  const double m = sum / (double)P.K;
  double sq = 0.0;
  for (int r = 0; r < P.K; ++r) {
    const double d = (double)cj[(size_t)P.elites[(size_t)r * P.E + e] * step] - m;
    sq += d * d;
  }
  store_fit(P, j, e, k, m, sq / (double)P.K);
}

// The sum over the whole workgroup of `acc` per component k = tid mod rowp
// (block_row_reduce), handed to every thread.
__device__ __forceinline__ double block_row_sum(double acc, double* part, int tid, int rowp) {
  qs::block_row_reduce(acc, part, tid, rowp);
  const double total = part[tid & (rowp - 1)];
  __syncthreads();   // part is used again
  return total;
}

// One workgroup per (env, step): thread t holds component k = t mod rowp of elite
// group g = t / rowp and strides over the ranks by the group count.
__global__ __launch_bounds__(qs::kCemBlockThreads) void cem_refit_block_kernel(RefitParams P) {
  __shared__ double part[qs::kCemBlockThreads];
  __shared__ int32_t sh_el[qs::kCemMaxElites];
  const int e = blockIdx.x % P.E, j = blockIdx.x / P.E, tid = threadIdx.x;
  if (tid < P.K) sh_el[tid] = P.elites[(size_t)tid * P.E + e];
  __syncthreads();
  const int rowp = P.rowp, k = tid & (rowp - 1), g = tid / rowp, G = qs::kCemBlockThreads / rowp;
  const size_t step = (size_t)P.E * P.row;
  const float* cj = P.cand + (size_t)j * P.C * step + (size_t)e * P.row;
  double acc = 0.0;
  if (blockIdx.x == 0 && tid == 0 && P.kept) *P.kept_n = P.keep;
  if (k < P.row) {
#pragma unroll 4
    for (int r = g; r < P.K; r += G) {
      const float x = cj[(size_t)sh_el[r] * step + k];
      if (r < P.keep) P.kept[((size_t)j * P.keep + r) * step + (size_t)e * P.row + k] = x;   // (keep = 0 without elite memory)
      acc += (double)x;
    }
  }
  const double m = block_row_sum(acc, part, tid, rowp) / (double)P.K;
  acc = 0.0;
  if (k < P.row) {
#pragma unroll 4
    for (int r = g; r < P.K; r += G) {
      const double d = (double)cj[(size_t)sh_el[r] * step + k] - m;
      acc += d * d;
    }
  }
  const double v = block_row_sum(acc, part, tid, rowp) / (double)P.K;
  if (tid < P.row) store_fit(P, j, e, tid, m, v);
}

// ---- finish: one thread per (e, d, a) column walks the steps upward, so nobody
// reads a step another thread has overwritten -------------------------------------
__global__ __launch_bounds__(qs::kCemThreads) void cem_finish_kernel(FinishParams P) {
  const uint64_t t = (uint64_t)blockIdx.x * qs::kCemThreads + threadIdx.x;
  if (t == 0) *P.tick += 1;
  if (t >= P.col) {   // the threads past the mean's columns walk the elite memory's
    const uint64_t u = t - P.col;
    if (!P.kept || u >= P.kept_col) return;
    for (int j = 0; j + 1 < P.n; ++j) P.kept[(size_t)j * P.kept_col + u] = P.kept[(size_t)(j + 1) * P.kept_col + u];
    return;
  }
  float cur = P.mean[t];
  P.action[t] = cur;
  for (int j = 0; j + 1 < P.n; ++j) {
    cur = P.mean[(size_t)(j + 1) * P.col + t];
    P.mean[(size_t)j * P.col + t] = cur;
  }
}

}  // namespace

struct qs_cem : qs::PlannerBase {
  qs_cem_spec spec;
  qs::CemVariant variant;
  qs::CemGrids grids;
  uint64_t bytes[qs::kCemBufs];
  void* buf[qs::kCemBufs];
};

namespace {

int begin_impl(qs_cem* p, hipStream_t st) {
  FillParams P;
  P.std = (float*)p->buf[qs::kCemStd];
  P.total = p->bytes[qs::kCemStd] / 4u;
  P.A = p->A;
  for (int a = 0; a < 4; ++a) P.sigma[a] = p->spec.sigma[a];
  hipLaunchKernelGGL(cem_fill_kernel, dim3(p->grids.fill), dim3(qs::kCemThreads), 0, st, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

// The shared sample kernel round the mean, its spread from `std`: tag 4 and the iteration.
int sample_impl(qs_cem* p, int iteration, hipStream_t st) {
  qs::SampleParams<StdMem> P;
  P.mean = (const float*)p->buf[qs::kCemMean];
  P.spread.std = (const float*)p->buf[qs::kCemStd];
  P.cand = (float*)p->buf[qs::kCemCandidates];
  P.tick = (const uint64_t*)p->buf[qs::kCemTick];
  P.k0 = (uint32_t)p->spec.seed; P.k1 = (uint32_t)(p->spec.seed >> 32);
  P.genv0 = (uint32_t)p->info.env_offset;
  P.tag = (uint32_t)qs::kCemTag; P.iter = (uint32_t)iteration;
  P.n = p->n; P.C = p->C; P.E = p->E; P.D = p->D; P.A = p->A;
  P.lo = p->spec.lo; P.hi = p->spec.hi;
  if (const qs::SamplingState* s = p->sampling; s && s->keep > 0) {   // candidates 1 .. *kept_n: the elite memory
    P.kept = s->kept;
    P.kept_n = s->kept_n;
    P.keep = (uint32_t)s->keep;
  }
  if (int rc = qs::planner_launch_sample(p, P, p->grids.sample, st)) return rc;   // (serial in j with a correlated sampling spec)
  return qs::prior_inject(p, P.cand, st);   // (nothing without a prior)
}

// The prior stage, keyed as the sample is: once per tick, whatever the iteration.
int prior_impl(qs_cem* p, void* stream) {
  return qs::prior_rollout("qs_prior_cem_rollout", p, p->spec.seed, (const uint64_t*)p->buf[qs::kCemTick], p->spec.lo,
                           p->spec.hi, stream);
}

int refit_impl(qs_cem* p, int iteration, hipStream_t st) {
  SelectParams S;
  S.ret = p->scores(p->buf[qs::kCemRet]);
  S.first_done = (const int32_t*)p->buf[qs::kCemFirstDone];
  S.elites = (int32_t*)p->buf[qs::kCemElites];
  S.iter_best = (double*)p->buf[qs::kCemIterBest] + (size_t)iteration * (size_t)p->units();
  S.penalty = p->spec.done_penalty;
  S.n = p->n; S.C = p->C; S.K = p->spec.elites; S.E = p->units();
  S.index_bytes = qs::cem_index_bytes(p->C);
  S.fd_div = p->fd_div();
  RefitParams R;
  R.cand = (const float*)p->buf[qs::kCemCandidates];
  R.elites = (const int32_t*)p->buf[qs::kCemElites];
  R.mean = (float*)p->buf[qs::kCemMean];
  R.std = (float*)p->buf[qs::kCemStd];
  R.alpha = p->spec.alpha;
  R.n = S.n; R.C = S.C; R.K = S.K; R.E = S.E; R.A = p->A;
  R.row = p->row();
  R.rowp = qs::mppi_row_pow2(R.row);
  for (int a = 0; a < 4; ++a) { R.sigma[a] = p->spec.sigma[a]; R.sigma_min[a] = p->spec.sigma_min[a]; }
  const qs::SamplingState* smp = p->sampling;
  const bool keeps = smp && smp->keep > 0;
  R.kept = keeps ? smp->kept : nullptr;
  R.kept_n = keeps ? smp->kept_n : nullptr;
  R.keep = keeps ? smp->keep : 0;
  if (p->variant == qs::kCemPerBlock) {
    hipLaunchKernelGGL(cem_select_block_kernel, dim3(p->grids.select), dim3(qs::kCemBlockThreads), 0, st, S);
    PLANNER_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cem_refit_block_kernel, dim3(p->grids.refit), dim3(qs::kCemBlockThreads), 0, st, R);
  } else {
    hipLaunchKernelGGL(cem_select_thread_kernel, dim3(p->grids.select), dim3(qs::kCemThreads), 0, st, S);
    PLANNER_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cem_refit_thread_kernel, dim3(p->grids.refit), dim3(qs::kCemThreads), 0, st, R);
  }
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

int finish_impl(qs_cem* p, hipStream_t st) {
  FinishParams P;
  P.mean = (float*)p->buf[qs::kCemMean];
  P.action = (float*)p->buf[qs::kCemAction];
  P.tick = (uint64_t*)p->buf[qs::kCemTick];
  P.col = p->bytes[qs::kCemAction] / 4u;
  P.n = p->n;
  const qs::SamplingState* smp = p->sampling;
  const bool keeps = smp && smp->keep > 0;
  P.kept = keeps ? smp->kept : nullptr;
  P.kept_col = keeps ? (uint64_t)smp->keep * P.col : 0;
  // with elite memory the grid also covers kept's columns: the launch count does not change
  const uint32_t grid = keeps ? qs::sampling_finish_grid(smp->keep, p->E, p->D, p->A) : p->grids.finish;
  hipLaunchKernelGGL(cem_finish_kernel, dim3(grid), dim3(qs::kCemThreads), 0, st, P);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

int bad_iteration(const qs_cem* p, int iteration, const char* who) {
  return qs::set_last_error(QS_E_INVALID, std::string(who) + ": iteration = " + std::to_string(iteration) +
                                              " is outside 0 .. iterations - 1 = " + std::to_string(p->spec.iterations - 1));
}

}  // namespace

namespace {
int create_impl(const char* who, bool per_drone, qs_handle* h, const qs_cem_spec* spec, qs_cem** out) {
  const std::string w = std::string(who) + ": ";
  using qs::set_last_error;
  qs_dims d;
  if (int rc = qs::planner_check_spec(who, "mean", h, spec, out, &d)) return rc;
  if (spec->elites < 1 || spec->elites > spec->candidates || spec->elites > qs::kCemMaxElites)
    return set_last_error(QS_E_INVALID, w + "elites = " + std::to_string(spec->elites) +
                                            " is outside 1 .. min(candidates, " + std::to_string(qs::kCemMaxElites) + ")");
  if (spec->iterations < 1 || spec->iterations > qs::kCemMaxIterations)
    return set_last_error(QS_E_INVALID, w + "iterations = " + std::to_string(spec->iterations) +
                                            " is outside 1 .. " + std::to_string(qs::kCemMaxIterations));
  for (int a = 0; a < d.act_dim && a < 4; ++a) {
    if (!(spec->sigma_min[a] >= 0.0f) || !std::isfinite(spec->sigma_min[a]))
      return set_last_error(QS_E_INVALID, w + "sigma_min[" + std::to_string(a) + "] must be finite and >= 0");
    if (spec->sigma_min[a] > spec->sigma[a])
      return set_last_error(QS_E_INVALID, w + "sigma_min[" + std::to_string(a) + "] is above sigma[" +
                                              std::to_string(a) + "]");
  }
  if (!(spec->alpha >= 0.0) || !(spec->alpha < 1.0))
    return set_last_error(QS_E_INVALID, w + "alpha must be in [0, 1)");
  qs_cem* p = qs::planner_new<qs_cem>(who, h, *spec, d);
  if (!p) return QS_E_NOMEM;
  p->per_drone = per_drone;
  const qs::CemShape shape{p->n, p->C, spec->elites, spec->iterations, p->E, p->D, p->A};
  if (per_drone ? !qs::cem_pd_sizes(shape, p->bytes, &p->ret_agent_bytes) : !qs::cem_sizes(shape, p->bytes))
    return qs::planner_too_large(who, p);
  const qs::CemShape ushape = per_drone ? qs::cem_pd_shape(shape) : shape;   // the units and rows of select and refit
  p->variant = qs::cem_variant(ushape.E, ushape.C, ushape.D * ushape.A);
  p->grids = qs::cem_grids(ushape, p->variant);
  if (int rc = qs::planner_alloc(who, p, qs::kCemCandidates)) return rc;
  *out = p;
  return QS_OK;
}
}  // namespace

extern "C" {

int qs_cem_create(qs_handle* h, const qs_cem_spec* spec, qs_cem** out) {
  return create_impl("qs_cem_create", false, h, spec, out);
}

int qs_pd_cem_create(qs_handle* h, const qs_cem_spec* spec, qs_cem** out) {
  return create_impl("qs_pd_cem_create", true, h, spec, out);
}

int qs_pd_cem_ret_agent(const qs_cem* p, double** out) { return qs::planner_ret_agent("qs_pd_cem_ret_agent", p, out); }

int qs_cem_destroy(qs_cem* p) { return qs::planner_destroy(p); }

int qs_cem_buffers(const qs_cem* p, qs_cem_bufs* out) {
  if (!p || !out) return qs::set_last_error(QS_E_INVALID, "qs_cem_buffers: null argument");
  out->mean = (float*)p->buf[qs::kCemMean];
  out->std = (float*)p->buf[qs::kCemStd];
  out->candidates = (float*)p->buf[qs::kCemCandidates];
  out->ret = (double*)p->buf[qs::kCemRet];
  out->first_done = (int32_t*)p->buf[qs::kCemFirstDone];
  out->elites = (int32_t*)p->buf[qs::kCemElites];
  out->iter_best = (double*)p->buf[qs::kCemIterBest];
  out->action = (float*)p->buf[qs::kCemAction];
  out->tick = (uint64_t*)p->buf[qs::kCemTick];
  return QS_OK;
}

int qs_cem_reset(qs_cem* p, const float* mean, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_reset: null planner");
  if (int rc = qs::planner_reset(p, qs::kCemMean, qs::kCemTick, mean, (hipStream_t)stream)) return rc;
  if (p->sampling && p->sampling->kept_n)   // the elite memory starts empty again
    PLANNER_HIP_TRY(hipMemsetAsync(p->sampling->kept_n, 0, 4, (hipStream_t)stream));
  return QS_OK;
}

int qs_cem_begin(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_begin: null planner");
  return begin_impl(p, (hipStream_t)stream);
}

int qs_cem_sample(qs_cem* p, int iteration, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_sample: null planner");
  if (iteration < 0 || iteration >= p->spec.iterations) return bad_iteration(p, iteration, "qs_cem_sample");
  return sample_impl(p, iteration, (hipStream_t)stream);
}

int qs_cem_refit(qs_cem* p, int iteration, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_refit: null planner");
  if (iteration < 0 || iteration >= p->spec.iterations) return bad_iteration(p, iteration, "qs_cem_refit");
  return refit_impl(p, iteration, (hipStream_t)stream);
}

int qs_cem_finish(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_finish: null planner");
  return finish_impl(p, (hipStream_t)stream);
}

int qs_value_cem_set(qs_cem* p, const qs_value_spec* spec) { return qs::value_attach("qs_value_cem_set", p, spec); }

int qs_value_cem_buffers(const qs_cem* p, float** last_obs, float** value, void** rewards) {
  return qs::value_buffers("qs_value_cem_buffers", p, last_obs, value, rewards);
}

int qs_value_cem_score(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_value_cem_score: null planner");
  if (int rc = qs::planner_ready("qs_value_cem_score", p)) return rc;
  return qs::value_score(p, p->buf[qs::kCemRet], p->buf[qs::kCemFirstDone], stream);
}

int qs_prior_cem_set(qs_cem* p, const qs_prior_spec* spec) { return qs::prior_attach("qs_prior_cem_set", p, spec); }

int qs_prior_cem_buffers(const qs_cem* p, float** prior_actions, float** prior_obs) {
  return qs::prior_buffers("qs_prior_cem_buffers", p, prior_actions, prior_obs);
}

int qs_prior_cem_rollout(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_prior_cem_rollout: null planner");
  if (int rc = qs::planner_ready("qs_prior_cem_rollout", p)) return rc;
  return prior_impl(p, stream);
}

int qs_avoid_cem_set(qs_cem* p, const qs_avoid_spec* spec) { return qs::avoid_attach("qs_avoid_cem_set", p, spec); }

int qs_avoid_cem_buffers(const qs_cem* p, double** cost_agent, double** ret_agent) {
  return qs::track_buffers("qs_avoid_cem_buffers", p, cost_agent, ret_agent);
}

int qs_avoid_cem_score(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_avoid_cem_score: null planner");
  if (int rc = qs::planner_ready("qs_avoid_cem_score", p)) return rc;
  return qs::planner_score(p, p->buf[qs::kCemRet], p->buf[qs::kCemFirstDone], stream);
}

int qs_track_cem_set(qs_cem* p, const qs_track_spec* spec) { return qs::track_attach("qs_track_cem_set", p, spec); }

int qs_track_cem_buffers(const qs_cem* p, double** cost_agent, double** ret_agent) {
  return qs::track_buffers("qs_track_cem_buffers", p, cost_agent, ret_agent);
}

int qs_track_cem_score(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_track_cem_score: null planner");
  if (int rc = qs::planner_ready("qs_track_cem_score", p)) return rc;
  return qs::planner_score(p, p->buf[qs::kCemRet], p->buf[qs::kCemFirstDone], stream);
}

int qs_sampling_cem_set(qs_cem* p, const qs_sampling_spec* spec) {
  return qs::sampling_attach("qs_sampling_cem_set", p, qs::kSamplingCem, p ? p->spec.elites : 0, spec);
}

int qs_sampling_cem_buffers(const qs_cem* p, float** kept, int32_t** kept_n) {
  if (!p || !kept || !kept_n) return qs::set_last_error(QS_E_INVALID, "qs_sampling_cem_buffers: null argument");
  *kept = p->sampling ? p->sampling->kept : nullptr;
  *kept_n = p->sampling ? p->sampling->kept_n : nullptr;
  return QS_OK;
}

int qs_cem_plan(qs_cem* p, void* stream) {
  if (!p) return qs::set_last_error(QS_E_INVALID, "qs_cem_plan: null planner");
  if (int rc = qs::planner_ready("qs_cem_plan", p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = begin_impl(p, st)) return rc;
  if (p->prior)
    if (int rc = prior_impl(p, stream)) return rc;
  for (int i = 0; i < p->spec.iterations; ++i) {
    if (int rc = sample_impl(p, i, st)) return rc;
    if (int rc = qs::value_score(p, p->buf[qs::kCemRet], p->buf[qs::kCemFirstDone], stream)) return rc;
    if (int rc = refit_impl(p, i, st)) return rc;
  }
  return finish_impl(p, st);
}

}  // extern "C"
