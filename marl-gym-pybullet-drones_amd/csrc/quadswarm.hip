// quadswarm.hip — host side of the MI355X quadrotor-swarm step: the C-ABI of
// include/quadswarm.h (handle, state buffers, launches).  The device code is
// csrc/step_kernel.h; the kernels are instantiated per task family in
// step_mh.hip / step_spiral.hip / step_marl.hip (single step), their
// *_fused.hip twins (several control steps per launch), step_mh_seq.hip /
// step_spiral_seq.hip (the same over caller-supplied actions), step_mh_score.hip /
// step_spiral_score.hip (branch rollouts that leave the handle alone),
// step_mh_branch.hip / step_spiral_branch.hip (the same on a branch set's state) and
// step_mh_hot.hip (MultiHover's shape-specialised multi-step instances).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <new>

#include "quadswarm.h"
#include "step_launch.h"
#include "step_fuse.h"
#include "step_score.h"
#include "track_sizes.h"
#include "avoid_sizes.h"
#include "step_branch.h"
#include "step_trunc.h"
#include "planner_link.h"

static_assert(qs::kFuseMax == qs::kMaxFuse, "step_fuse.h and step_kernel.h disagree on the fusion depth");
static_assert(qs::kObsPipeMaxRow == qs::kObsPipeMaxO && qs::kObsPipeRows == qs::kBlock,
              "step_fuse.h and step_kernel.h disagree on the fast obs path's shape");
static_assert(qs::kSeqStepBytes == qs::kBlock * (int)sizeof(float), "step_fuse.h and step_kernel.h disagree on an action row's LDS");
static_assert(qs::kHotTask == QS_TASK_MULTIHOVER && qs::kHotAct == QS_ACT_ONE_D_PID && qs::kHotPhysA == QS_PHYS_PYB &&
                  qs::kHotPhysB == QS_PHYS_DYN && qs::kHotBadFlags == (QS_FLAG_NO_AUTORESET | QS_FLAG_CF2P),
              "step_fuse.h restates quadswarm.h's values for the hot shape");
static_assert(qs::kHotDrones == qs::kHotD && qs::kHotEnvs == qs::kBlock / qs::kHotD && qs::kFuseOuts == 7,
              "step_fuse.h and step_kernel.h disagree on the hot shape");

static_assert(qs::kScoreMaxSteps == qs::kMaxFuse && qs::kScoreStepBytes == qs::kSeqStepBytes &&
                  qs::kScoreStepOuts == qs::kFuseOuts,
              "step_score.h disagrees with step_kernel.h / step_fuse.h on a launch's steps, action rows or outputs");

static_assert(qs::kBranchEnvRec == qs::kEnvRec, "step_branch.h disagrees with step_kernel.h on an env record's words");

namespace qs {
// Calibration kernel: dword per lane, grid-stride (MI355X_MICROARCH §HBM).
__global__ void calib_copy_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}

// ------------------------------------------------------------ branch sets: fork and select
// One kernel moves every block of a branch set (qs_branch_fork, qs_branch_select).
// A block is `rows` rows of `cand` candidates of `row` units each, a unit 16 or 4
// bytes: agent state [field][c][E · D], env records [1][c][E], history
// [slot][c][E · D · A], and the accumulators likewise.  dst[r][c][l] = src[r][pc][l]:
//   fork   (src_cand = 1): pc = 0, the handle's row tiled to the C candidates;
//   select (src_cand = C): pc = parent[c][e] where that is a candidate, else c, e the
//          env unit l lies in (`per_env` units to an env; a 16-byte unit is chosen
//          only where it does not straddle two envs);
//   src = NULL: zeros.
// Lane i of a wave moves unit i of a row, so every load and store is a whole
// coalesced line of the [field][agent] layout; src and dst never alias (select
// gathers into the set's shadow allocation, which is then copied back whole, so no
// candidate reads what another has already overwritten).  Units of a block stay
// below 2^31 (step_branch.h), so the index arithmetic is 32-bit.
struct BranchSeg {
  const void* src;
  void* dst;
  unsigned row, rows, cand, src_cand, per_env, unit;
};
struct BranchMove {
  BranchSeg seg[kBranchBlocks];
  const int32_t* parent;   // [C][E] (select) or NULL
  unsigned C, E;
};
template <class U> __device__ __forceinline__ void branch_move_seg(const BranchSeg& g, const int32_t* parent, unsigned C, unsigned E) {
  const unsigned per_cand = g.row, total = g.rows * g.cand * per_cand;
  const U* const src = static_cast<const U*>(g.src);
  U* const dst = static_cast<U*>(g.dst);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    U v{};
    if (src) {
      const unsigned rc = i / per_cand, l = i - rc * per_cand;
      const unsigned r = rc / g.cand, c = rc - r * g.cand;
      unsigned pc = 0;
      if (g.src_cand != 1) {
        const int32_t p = parent[c * E + l / g.per_env];
        pc = (p >= 0 && (unsigned)p < C) ? (unsigned)p : c;
      }
      v = src[(size_t)(r * g.src_cand + pc) * per_cand + l];
    }
    dst[i] = v;
  }
}
__global__ void __launch_bounds__(256) branch_move_kernel(BranchMove m) {
  const BranchSeg& g = m.seg[blockIdx.y];
  if (g.unit == 16) branch_move_seg<uint4>(g, m.parent, m.C, m.E);
  else branch_move_seg<uint32_t>(g, m.parent, m.C, m.E);
}

// ------------------------------------------------------------ episode log query
// qs_episode_log selects the newest `cap` records of the per-env rings on the
// device, so that O(cap) records — not the E·R ring slots — cross to the host.
// An env's ring holds its last min(n, R) episodes (n = its logged count) in
// slots (n − min(n, R)) … (n − 1) mod R.
constexpr int kLogBins = 4096;   // seq-distance bins below the newest seq (the last one: ≥ 4095)
struct LogWork {
  unsigned long long total;      // Σ_e n_e
  long long maxseq;              // newest seq over every ring
  unsigned int nsel;             // records compacted by log_select_kernel
  unsigned int pad;
  unsigned int hist[kLogBins];   // live ring slots per (maxseq − seq) bin
};

__device__ __forceinline__ long long env_logged(const int32_t* env, int e) {
  return env[(size_t)e * kEnvRec + kEnvLogWord];
}

// total and newest seq: block sums / maxima, then one global atomic per block
__global__ void __launch_bounds__(256) log_scan_kernel(const int32_t* __restrict__ env,
                                                       const qs_episode_rec* __restrict__ log, int E, int R,
                                                       LogWork* w) {
  __shared__ unsigned long long ssum[4];
  __shared__ long long smax[4];
  const int e = blockIdx.x * 256 + threadIdx.x;
  unsigned long long n = 0;
  long long mx = -1;
  if (e < E) {
    const long long c = env_logged(env, e);
    n = (unsigned long long)c;
    // every live slot (seq grows along a ring, but qs_state_io may rewrite the counters)
    for (long long i = c > R ? c - R : 0; i < c; ++i) mx = max(mx, log[(size_t)e * R + (size_t)(i % R)].seq);
  }
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = n; smax[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = ssum[0] + ssum[1] + ssum[2] + ssum[3];
    const long long m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    if (t) atomicAdd(&w->total, t);
    if (m >= 0) atomicMax(&w->maxseq, m);
  }
}

// histogram of (maxseq − seq) over the live ring slots: LDS bins, only the
// non-empty ones flushed
__global__ void __launch_bounds__(256) log_hist_kernel(const int32_t* __restrict__ env,
                                                       const qs_episode_rec* __restrict__ log, int E, int R,
                                                       LogWork* w) {
  __shared__ unsigned int h[kLogBins];
  for (int b = threadIdx.x; b < kLogBins; b += 256) h[b] = 0;
  __syncthreads();
  const int e = blockIdx.x * 256 + threadIdx.x;
  const long long top = w->maxseq;
  if (e < E) {
    const long long n = env_logged(env, e);
    for (long long i = n > R ? n - R : 0; i < n; ++i) {
      const long long d = max(0LL, top - log[(size_t)e * R + (size_t)(i % R)].seq);
      atomicAdd(&h[d < kLogBins - 1 ? (int)d : kLogBins - 1], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kLogBins; b += 256)
    if (h[b]) atomicAdd(&w->hist[b], h[b]);
}

// every live record with seq ≥ thr, in no particular order (the host orders them)
__global__ void __launch_bounds__(256) log_select_kernel(const int32_t* __restrict__ env,
                                                         const qs_episode_rec* __restrict__ log, int E, int R,
                                                         long long thr, qs_episode_rec* __restrict__ out,
                                                         unsigned int out_cap, LogWork* w) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const long long n = env_logged(env, e);
  for (long long i = n > R ? n - R : 0; i < n; ++i) {
    const qs_episode_rec r = log[(size_t)e * R + (size_t)(i % R)];
    if (r.seq < thr) continue;
    const unsigned int k = atomicAdd(&w->nsel, 1u);
    if (k < out_cap) out[k] = r;
  }
}

}  // namespace qs

// ===========================================================================
// Host side: the C-ABI.
// ===========================================================================
namespace {
thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }
#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) return fail(QS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// cf2x.urdf + BaseAviary.py:117-128 (same values as the oracle's Consts).
struct HostConsts {
  double G = 9.8, M = 0.027, L = 0.0397, T2W = 2.25, IXX = 1.4e-5, IYY = 1.4e-5, IZZ = 2.17e-5;
  double KF = 3.16e-10, KM = 7.94e-12, COLL_H = 0.025, COLL_Z_OFF = 0.0, MAX_SPEED_KMH = 30.0;
  double GND_EFF_COEFF = 11.36859, PROP_RADIUS = 2.31348e-2, DRAG_XY = 9.1785e-7, DRAG_Z = 10.311e-7;
  double DW1 = 2267.18, DW2 = 0.16, DW3 = -0.11;
};
}  // namespace

struct qs_handle {
  qs_spec spec;
  qs_dims dims;
  int device = 0;
  void* st = nullptr;          // agent SoA (real)
  int32_t* env = nullptr;      // per-env records [E][qs::kEnvRec] (counters + episode return)
  float* hist = nullptr;
  void* orig = nullptr;        // [D][3] real
  qs_episode_rec* log = nullptr;
  int log_per_env = 0;
  int* err = nullptr;
  unsigned long long* stamps = nullptr;   // dev-only (QS_STAMPS)
  int* rq = nullptr;            // deferred reset-search queue (header + one 128-B record per env), MultiHover layouts that can reject
  int32_t* rpre = nullptr;      // [E] each env's precomputed next-episode reset search (qs::kPreFound)
  bool reject_free = false;     // MultiHover layout whose reset draws can never be rejected
  int num_cu = 256;             // compute units of the device (LDS residency plan)
  qs::LogWork* logw = nullptr;  // qs_episode_log's device scratch
  qs_episode_rec* log_sel = nullptr;   // its compacted records (log_sel_cap slots, grown on demand)
  size_t log_sel_cap = 0;
  uint64_t seed = 0;
  bool reset_done = false;
  std::vector<double> orig_host;
  // Steps per launch of the synthetic-policy rollout (QS_MAX_FUSED_STEPS, 1 ..
  // qs::kMaxFuse; 1 = every step its own launch).  `fuse`: the kernel node of a
  // stream capture that the last qs_step made and the next one may grow
  // (step_fuse.h), with the launch parameters the node holds.
  int fuse_depth = 1;
  // Multi-step launches: per-env reward / done / reset flags inside the wave (DPP,
  // ballots) where an env is 2, 4, 8 or 16 lanes; QS_WAVE_REDUCE=0 keeps them on the
  // LDS path (the A/B switch)
  bool wave_reduce = true;
  // Multi-step launches of the shape qs::hot_shape_ok accepts run the specialised
  // instance (step_mh_hot.hip); QS_HOT_SHAPE=0 keeps them on the general one (the
  // A/B switch).  launches[]: multi-step launches made so far on the general [0]
  // and on the specialised [1] instance (qs_launch_counts); a capture's kernel
  // node counts once, under the instance it names after its last append
  // (fuse_kind: which one that is for the node of h->fuse, -1 before it holds two steps).
  bool hot_shape = true;
  int64_t launches[2] = {0, 0};
  int fuse_kind = -1;
  // A hot-shape launch goes on past its distinct output sets while the further
  // steps write them again in order (step_fuse.h, can_wrap; the ring instance,
  // step_mh_ring.hip); QS_RING_LAUNCH=0 cuts such a launch as before (the A/B
  // switch), QS_RING_MAX_STEPS (1 .. qs::kRingMaxSteps) caps its steps.  ring[]:
  // ring launches made so far and the steps they held (qs_ring_counts); a
  // capture's node counts once, with the steps it holds after its last wrap
  // (fuse_ring_steps: how many of ring[1] are the node's of h->fuse).
  bool ring_launch = true;
  int ring_max = qs::kRingMaxSteps;
  int64_t ring[2] = {0, 0};
  int fuse_ring_steps = 0;
  qs::FuseGroup fuse;
  qs::ParamsMany<float> fuse_pf;
  qs::ParamsMany<double> fuse_pd;
};

// Envs per one-wave workgroup: ⌊64/D⌋, a launch parameter (P.EPB).  A dev build
// may halve it while the grid holds fewer than kEpbWaves waves per SIMD (at
// most QS_EPB_HALVINGS times), to overlap more waves' latency chains on an
// under-filled grid (Spiral C4: 683 waves of 12 envs for 1 024 SIMDs) — but
// every wave pays the same load → PID → substeps → reward → store chain, and
// one halving made C4 11.6 → 18.2 µs (as round 2's probe found), so the
// default is none.  Results do not depend on it: every per-env quantity is
// formed inside the env's own lanes.
#ifndef QS_EPB_HALVINGS
#define QS_EPB_HALVINGS 0   // measured: one halving made Spiral C4 11.6 -> 18.2 µs; dev builds probe it
#endif
#ifndef QS_EPB_WAVES
#define QS_EPB_WAVES 2   // (dev builds: the waves per SIMD below which a halving applies)
#endif
static constexpr int kEpbWaves = QS_EPB_WAVES;
static int envs_per_wave(const qs_handle* h) {
  const int E = h->spec.num_envs, simds = 4 * h->num_cu;
  int epb = qs::kBlock / h->spec.num_drones;
  for (int k = 0; k < QS_EPB_HALVINGS && epb > 1 && (E + epb - 1) / epb < kEpbWaves * simds; ++k) epb = (epb + 1) / 2;
  return epb;
}

template <class T> static void fill_params(const qs_handle* h, qs::Params<T>& P) {
  const qs_spec& s = h->spec;
  std::memset(&P, 0, sizeof(P));
  P.E = s.num_envs; P.D = s.num_drones; P.N = h->dims.num_agents; P.O = h->dims.obs_dim;
  P.H = h->dims.hist_len; P.S = h->dims.substeps;
  P.EPB = envs_per_wave(h);
  P.aux = s.aux_forces; P.flags = s.flags; P.pyb_freq = s.pyb_freq; P.task = s.task;
  P.ep_len_sec = s.episode_len_sec;
  P.trunc_at = qs::trunc_threshold(s.pyb_freq, s.episode_len_sec);
  P.wave_reduce = h->wave_reduce ? 1 : 0;
  P.k0 = (uint32_t)h->seed; P.k1 = (uint32_t)(h->seed >> 32);
  P.env_offset = s.env_offset;
  P.reset_queue = h->rq;
  P.reset_pre = h->rpre;
  P.reject_free = h->reject_free ? 1 : 0;
  const double dt = 1.0 / s.pyb_freq;
  P.dt = T(dt); P.hdt = T(dt / 2); P.hdt2 = T((dt / 2) * (dt / 2)); P.ctrl_dt = T(1.0 / s.ctrl_freq); P.ctrl_hz = T(s.ctrl_freq);
  P.sp_R = T(s.spiral_radius); P.sp_OMEGA = T(2 * M_PI / s.spiral_period); P.sp_VZ = T(s.height_rate);
  P.sp_cx = T(s.target_center[0]); P.sp_cy = T(s.target_center[1]); P.sp_cz = T(s.target_center[2]);
  P.st = (T*)h->st; P.env = h->env; P.hist = h->hist; P.orig_xyz = (const T*)h->orig;
  P.log = h->log; P.log_per_env = h->log_per_env; P.err = h->err;
  P.stamps = h->stamps;
}

// LDS per workgroup: the history prefetch image plus obs rows staged per pass.
// The staging is sized so that the launch's workgroups are resident at once:
// `resident` = ⌈grid / CUs⌉ of them must share a CU's 160 KB (else the grid runs
// in rounds, each paying the whole per-wave latency again: Spiral C4's 683
// one-wave workgroups at 61 KB each ran as 512 + 171, 17.5 µs → 12.0 µs).  When
// the whole grid cannot be resident even with fewer staged rows (MultiHover VEL:
// 15 KB of history per workgroup), full staging is kept — more passes of fewer
// rows cost more than the partial residency returns (C3-VEL 22.3 → 26.0 µs).
static constexpr size_t kLdsBytes = 160 * 1024, kLdsStatic = 8192, kLdsGrain = 512, kStageBudget = 48 * 1024;
static int lds_plan(const qs_dims& d, int epb, int resident, int* stage_rows, size_t* bytes) {
  const size_t hist = (size_t)d.hist_len * qs::kBlock * d.act_dim * sizeof(float);
  const size_t row = (size_t)d.obs_dim * sizeof(float);
  if (hist + row + kLdsStatic > kLdsBytes) return QS_E_INVALID;
  const int rows = epb * d.num_drones;
  size_t per = kLdsBytes / (size_t)std::max(1, std::min(resident, 32));   // a workgroup's share at full residency
  if (per < kLdsStatic + kLdsGrain + hist + row) per = kLdsBytes;          // unreachable: plain staging
  const size_t budget = std::min(kStageBudget, per - kLdsStatic - kLdsGrain - hist);
  *stage_rows = (int)std::max<size_t>(1, std::min<size_t>(rows, budget / row));
  *bytes = hist + (size_t)*stage_rows * row;
  return QS_OK;
}

// The instances with the compile-time control frequency (launch_one's `cf`, and
// not DroneModel.CF2P): they keep the action history in registers.
static bool fixed_ctrl_freq(const qs_spec& s) {
  return !(s.flags & QS_FLAG_CF2P) && s.pyb_freq == 240 && s.ctrl_freq == (s.task == QS_TASK_SPIRAL ? 48 : 30);
}
// Dynamic LDS of a FUSE = 2 launch, without its action rows: lds_plan's bytes,
// less the history image where the instance does not use it (step_kernel.h puts
// the action rows first, then the image if any, then the obs stage).
static size_t seq_lds_base(const qs_handle* h, size_t plan_bytes) {
  const size_t hist = (size_t)h->dims.hist_len * qs::kBlock * h->dims.act_dim * sizeof(float);
  return fixed_ctrl_freq(h->spec) ? plan_bytes - hist : plan_bytes;
}

// What a launch ran (or, select_only, would run): a graph kernel node's fields.
struct LaunchInfo {
  const void* fn = nullptr;
  int grid = 0;
  size_t lds = 0;
};

// What qs::hot_shape_ok judges, for a multi-step launch over P.io[0 .. P.nsteps-1]
// (P.nsteps <= qs::kMaxFuse; P.obs_pipe decided); masks: the steps' output masks.
template <class T>
static qs::HotShape hot_shape_of(const qs_handle* h, const qs::ParamsMany<T>& P, unsigned masks[qs::kMaxFuse]) {
  const qs_spec& s = h->spec;
  for (int j = 0; j < P.nsteps; ++j) {
    const qs::StepIO<T>& o = P.io[j];
    masks[j] = qs::out_mask(qs::FuseOuts{{o.obs, o.rew, o.term, o.trunc, o.tobs, o.reasons, o.act_out}});
  }
  return qs::HotShape{s.task, s.act_type, fixed_ctrl_freq(s), s.physics, s.aux_forces, s.flags, P.D, P.E, P.EPB,
                      P.reject_free != 0, P.reset_queue != nullptr, P.reset_pre != nullptr, P.wave_reduce != 0,
                      P.obs_pipe != 0};
}

// Grid, LDS plan (P.stage_rows) and the kernel of a launch; FUSE = 1: the
// multi-step instance over P.io[0 .. P.nsteps-1] (MODE_STEP, no trainer actions,
// no deferred reset queue: the callers see to that); FUSE = 2: the same over the
// actions P.act[0 .. P.nsteps-1], whose rows take LDS of their own (the caller
// has capped P.nsteps by seq_depth); FUSE = 3: the FUSE = 2 launch over P.E
// virtual envs (qs_score, P.nsteps within score_depth); FUSE = 4: that launch on a
// branch set's own blocks (qs_branch_advance); FUSE = 5: the FUSE = 3 launch with a
// tracking cost (qs_track_score); FUSE = 6: that launch with separation and obstacle
// terms (qs_avoid_score).  select_only: no launch.
template <class T, int FUSE>
static int launch_kernel(qs_handle* h, qs::KernelParams<T, FUSE>& P, hipStream_t st, LaunchInfo* info, bool select_only,
                         int* kind = nullptr) {
  const int grid = (P.E + P.EPB - 1) / P.EPB;
  size_t lds = 0;
  if (lds_plan(h->dims, P.EPB, (grid + h->num_cu - 1) / h->num_cu, &P.stage_rows, &lds) != QS_OK)
    return fail(QS_E_INVALID, "launch: action history does not fit in LDS (ctrl_freq too high)");
  const qs_spec& s = h->spec;
  if constexpr (FUSE != 0) {
    // the fast obs path, decided per launch (step_fuse.h); the instances with the
    // compile-time control frequency are the ones launch_one picks under `fixed_cf`
    const bool fixed_cf = fixed_ctrl_freq(s);
    const void* obs[qs::kMaxFuse];
    for (int j = 0; j < P.nsteps; ++j) obs[j] = P.io[j].obs;
    P.obs_pipe = qs::obs_pipe_ok(fixed_cf, P.stage_rows, P.EPB * P.D, P.O, obs, P.nsteps) ? 1 : 0;
    if constexpr (FUSE == 1) {
      // the shape-specialised instance, decided per launch over all its steps (so a
      // capture's node is re-decided, either way, each time a step joins it)
      unsigned masks[qs::kMaxFuse];
      const qs::HotShape hs = hot_shape_of(h, P, masks);
      const bool hot = h->hot_shape && qs::hot_shape_ok(hs, masks, P.nsteps);
      if (kind) *kind = hot ? 1 : 0;
      if (hot) {
        const void* fn = nullptr;
        qs::launch_hot<T>(s.physics, grid, lds, st, P, &fn, select_only);
        if (info) { info->fn = fn; info->grid = grid; info->lds = lds; }
        if (select_only) return QS_OK;
        HIP_TRY(hipGetLastError());
        h->launches[1] += 1;
        return QS_OK;
      }
    }
  }
  if constexpr (FUSE == 2 || FUSE == 3 || FUSE == 4 || FUSE == 5 || FUSE == 6) {
    lds = seq_lds_base(h, lds) + (size_t)P.nsteps * qs::kSeqStepBytes * (size_t)h->dims.act_dim;
    if (lds + kLdsStatic > kLdsBytes) return fail(QS_E_INVALID, "launch: the steps' action rows do not fit in LDS");
  }
  const void* fn = nullptr;
  bool ok;
  if (s.task == QS_TASK_MULTIHOVER)
    ok = qs::launch_task<T, QS_TASK_MULTIHOVER, FUSE>(s.act_type, grid, lds, st, P, s.ctrl_freq, s.pyb_freq, s.physics, &fn,
                                                      select_only);
  else if (s.task == QS_TASK_SPIRAL)
    ok = qs::launch_task<T, QS_TASK_SPIRAL, FUSE>(s.act_type, grid, lds, st, P, s.ctrl_freq, s.pyb_freq, s.physics, &fn,
                                                  select_only);
  else if constexpr (FUSE == 2 || FUSE == 3 || FUSE == 4 || FUSE == 5 || FUSE == 6)
    return fail(QS_E_INVALID, "launch: no action-sequence instances of the Flock / Meetup / LeaderFollower family");
  else
    ok = qs::launch_task<T, qs::kTaskMarl, FUSE>(s.act_type, grid, lds, st, P, s.ctrl_freq, s.pyb_freq, s.physics, &fn,
                                                 select_only);
  if (!ok) return fail(QS_E_INVALID, "launch: bad act_type");
  if (info) { info->fn = fn; info->grid = grid; info->lds = lds; }
  if (select_only) return QS_OK;
  HIP_TRY(hipGetLastError());
  if constexpr (FUSE == 1) h->launches[0] += 1;
  return QS_OK;
}

// A launch of P.nsteps (>= 2) control steps.  `kind`, if given, receives the
// instance chosen: 0 general, 1 shape-specialised.
template <class T> static int launch_many(qs_handle* h, qs::ParamsMany<T>& P, hipStream_t st, LaunchInfo* info = nullptr,
                                          bool select_only = false, int* kind = nullptr) {
  return launch_kernel<T, 1>(h, P, st, info, select_only, kind);
}

// A ring launch (step_fuse.h, can_wrap): `total` steps over the P.nsteps distinct
// output sets of P (the period), on the ring instance.  Grid, LDS plan, the fast
// obs path and the shape are decided over the distinct sets, as for the launch
// of those alone; R receives the arguments (what a graph kernel node holds).
// QS_E_INVALID if qs::ring_shape_ok refuses (the callers wrap only what it accepts).
template <class T> static int launch_ring(qs_handle* h, qs::ParamsMany<T>& P, int total, hipStream_t st, qs::ParamsRing<T>& R,
                                          LaunchInfo* info = nullptr, bool select_only = false) {
  LaunchInfo li;
  const int rc = launch_many(h, P, st, &li, /*select_only=*/true);
  if (rc != QS_OK) return rc;
  unsigned masks[qs::kMaxFuse];
  const qs::HotShape hs = hot_shape_of(h, P, masks);
  if (!h->hot_shape || !h->ring_launch || !qs::ring_shape_ok(hs, masks, P.nsteps, total))
    return fail(QS_E_INVALID, "launch: not a ring launch");
  std::memset(&R, 0, sizeof(R));
  static_cast<qs::ParamsMany<T>&>(R) = P;
  R.period = P.nsteps;
  R.nsteps = total;
  const void* fn = nullptr;
  qs::launch_ring<T>(h->spec.physics, li.grid, li.lds, st, R, &fn, select_only);
  if (info) { info->fn = fn; info->grid = li.grid; info->lds = li.lds; }
  if (select_only) return QS_OK;
  HIP_TRY(hipGetLastError());
  h->launches[1] += 1;
  h->ring[0] += 1;
  h->ring[1] += total;
  return QS_OK;
}
// Would the launch of P's distinct sets run the hot shape (so that it may wrap)?
template <class T> static bool ring_eligible(qs_handle* h, qs::ParamsMany<T>& P, hipStream_t st) {
  int kind = 0;
  return h->ring_launch && P.nsteps >= 2 && launch_many(h, P, st, nullptr, /*select_only=*/true, &kind) == QS_OK && kind == 1;
}

// Steps per launch of qs_step_seq: the handle's depth, capped where the action
// rows (LDS, step_fuse.h seq_depth_cap) would not leave the launch's workgroups
// resident at once.
static constexpr size_t kSeqLdsMax = 64 * 1024;
static int seq_depth(const qs_handle* h) {
  if (h->rq) return 1;   // the search launch sits between two steps of an env
  // Flock / Meetup / LeaderFollower: the multi-step instances of this family form
  // the env reward with other division / square-root expansions than the single
  // step (1 ulp apart), and qs_step_seq promises the single
  // steps' bits: single steps, and no FUSE = 2 instances of the family are built
  if (h->spec.task != QS_TASK_MULTIHOVER && h->spec.task != QS_TASK_SPIRAL) return 1;
  const int epb = envs_per_wave(h);
  const int grid = (h->spec.num_envs + epb - 1) / epb;
  const int resident = std::max(1, std::min((grid + h->num_cu - 1) / h->num_cu, 32));
  int stage_rows = 0;
  size_t plan = 0;
  if (lds_plan(h->dims, epb, resident, &stage_rows, &plan) != QS_OK) return 1;
  const size_t used = kLdsStatic + kLdsGrain + seq_lds_base(h, plan);
  // (a workgroup of these launches stays within kSeqLdsMax in all: none of the
  // project's measured launches has asked for more)
  const size_t share = std::min(kLdsBytes / (size_t)resident, kSeqLdsMax);
  return qs::seq_depth_cap(share > used ? share - used : 0, kSeqLdsMax > used ? kSeqLdsMax - used : 0, h->dims.act_dim,
                           h->fuse_depth);
}

template <class T> static int launch(qs_handle* h, qs::Params<T>& P, hipStream_t st, LaunchInfo* info = nullptr) {
  const int rc = launch_kernel<T, 0>(h, P, st, info, false);
  if (rc != QS_OK) return rc;
  if (P.reset_queue) {   // the envs whose try 0 was rejected (usually none)
    // Workgroups claim chunks of the queued envs' tries dynamically; kQueueWG
    // workgroups for the queue, then one per kPreEnvs envs (up to 4 096 envs,
    // grid-strided beyond) for the precomputed resets
    const int rgrid = qs::kQueueWG + std::min(4096 / qs::kPreEnvs, (P.E + qs::kPreEnvs - 1) / qs::kPreEnvs);
    hipLaunchKernelGGL(qs::reset_search_kernel<T>, dim3(rgrid), dim3(qs::kResetBlock), 0, st, P);
    HIP_TRY(hipGetLastError());
  }
  return QS_OK;
}

// The device code folds the CF2X constants as literals (qs::cf2x); re-derive
// them here from the URDF values exactly as the oracle does and refuse to run
// if any literal is not the correctly rounded value.
static int check_consts() {
  const HostConsts C;
  namespace K = qs::cf2x;
  const bool ok = K::G == C.G && K::M == C.M && K::L == C.L && K::KF == C.KF && K::KM == C.KM &&
                  K::IXX == C.IXX && K::IYY == C.IYY && K::IZZ == C.IZZ &&
                  K::L_SQRT2 == C.L / std::sqrt(2.0) &&
                  K::HOVER_RPM == std::sqrt(C.G * C.M / (4 * C.KF)) &&
                  K::SPEED_LIMIT == 0.03 * C.MAX_SPEED_KMH * (1000.0 / 3600.0) &&
                  K::DRAG_XY == C.DRAG_XY && K::DRAG_Z == C.DRAG_Z && K::GND_COEFF == C.GND_EFF_COEFF &&
                  K::PROP_R == C.PROP_RADIUS && K::DW1 == C.DW1 && K::DW2 == C.DW2 && K::DW3 == C.DW3;
  const double max_rpm = std::sqrt((C.T2W * C.G * C.M) / (4 * C.KF));
  const double max_thrust = 4 * C.KF * max_rpm * max_rpm;
  const double gnd_clip = 0.25 * C.PROP_RADIUS * std::sqrt((15 * max_rpm * max_rpm * C.KF * C.GND_EFF_COEFF) / max_thrust);
  if (!ok || K::GND_CLIP != gnd_clip) return fail(QS_E_INVALID, "qs_create: CF2X device constants disagree with the URDF derivation");
  // CF2P (QS_FLAG_CF2P): cf2p.urdf:12 inertia, props on the body axes at L (cf2p.urdf:42-79)
  using MP = qs::Model<true>;
  const bool okp = MP::IXX == 2.3951e-5 && MP::IYY == 2.3951e-5 && MP::IZZ == 3.2347e-5 && MP::PX[0] == C.L &&
                   MP::PY[1] == C.L && MP::PX[2] == -C.L && MP::PY[3] == -C.L && MP::PX[1] == 0 && MP::PY[0] == 0;
  if (!okp) return fail(QS_E_INVALID, "qs_create: CF2P device constants disagree with cf2p.urdf");
  return QS_OK;
}

// ---------------------------------------------------------------- stepping
template <class T> static qs::ParamsMany<T>& fuse_params(qs_handle* h) {
  if constexpr (sizeof(T) == 8) return h->fuse_pd;
  else return h->fuse_pf;
}
template <class T> static qs::StepIO<T> to_io(const qs_step_out& o) {
  return qs::StepIO<T>{o.obs, (T*)o.reward, o.terminated, o.truncated, o.terminal_obs, o.reasons, o.actions_out};
}
static qs::FuseOuts to_outs(const qs_step_out& o) {
  return qs::FuseOuts{{o.obs, o.reward, o.terminated, o.truncated, o.terminal_obs, o.reasons, o.actions_out}};
}
// bytes a step writes through each qs_step_out pointer (to_outs order)
static void out_sizes(const qs_handle* h, size_t b[qs::kFuseOuts]) {
  const qs_dims& d = h->dims;
  const size_t N = (size_t)d.num_agents, E = (size_t)d.num_envs, row = (size_t)d.obs_dim * sizeof(float);
  b[0] = N * row; b[1] = E * (size_t)d.precision; b[2] = E; b[3] = E; b[4] = N * row; b[5] = N;
  b[6] = N * (size_t)d.act_dim * sizeof(float);
}
template <class T> static void single_step_params(const qs_handle* h, qs::Params<T>& P, const float* actions,
                                                  const qs_step_out& o) {
  fill_params(h, P);
  P.mode = qs::MODE_STEP;
  P.act_in = actions; P.obs = o.obs; P.rew = (T*)o.reward; P.term = o.terminated; P.trunc = o.truncated;
  P.tobs = o.terminal_obs; P.reasons = o.reasons; P.act_out = o.actions_out;
}

struct CaptureState {
  bool active = false;
  unsigned long long id = 0;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
};
// The capture `st` is in, if any; a failed query counts as none.
static CaptureState capture_state(hipStream_t st) {
  CaptureState c;
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  hipGraph_t graph = nullptr;
  if (hipStreamGetCaptureInfo_v2(st, &status, &c.id, &graph, &c.deps, &c.ndeps) != hipSuccess) {
    (void)hipGetLastError();
    return CaptureState{};
  }
  c.active = status == hipStreamCaptureStatusActive;
  return c;
}

// qs_step on a capturing stream, synthetic policy: if the stream's capture still
// ends in the kernel node the previous qs_step made (h->fuse) and nothing else
// depends on that node, this step joins it: the node becomes the multi-step
// kernel over one more output set, and nothing is launched.  false: the caller
// takes the single launch (any doubt, any refusal of the runtime).
template <class T> static bool try_coalesce(qs_handle* h, const qs_step_out& o, hipStream_t st) {
  qs::FuseGroup& g = h->fuse;
  const CaptureState c = capture_state(st);
  if (!c.active || !g.same_capture(c.id, (void*)st)) return false;   // (ids first: the node of an ended capture may be gone)
  hipGraphNode_t node = (hipGraphNode_t)g.node;
  if (c.ndeps != 1 || c.deps[0] != node) return false;
  size_t dependents = 0;
  if (hipGraphNodeGetDependentNodes(node, nullptr, &dependents) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (dependents != 0) return false;
  const qs::FuseOuts fo = to_outs(o);
  // a new output set while the node has not wrapped; else the set that is due in its ring
  const bool grow = g.period == 0 && g.can_append(fo, h->fuse_depth);
  if (!grow && !(h->ring_launch && g.can_wrap(fo, h->fuse_depth, h->ring_max))) return false;
  qs::ParamsMany<T> P = fuse_params<T>(h);   // (P.nsteps counts the distinct sets)
  if (grow) {
    P.io[g.count] = to_io<T>(o);
    P.nsteps = g.count + 1;
  }
  LaunchInfo li;
  int kind = 0;
  qs::ParamsRing<T> R;
  void* args[1] = {&P};
  if (grow) {
    if (launch_many(h, P, st, &li, /*select_only=*/true, &kind) != QS_OK || !li.fn) return false;
  } else {   // the node moves to (or stays on) the ring instance; a shape that is not hot cuts here
    if (launch_ring(h, P, g.total + 1, st, R, &li, /*select_only=*/true) != QS_OK || !li.fn) return false;
    kind = 1;
    args[0] = &R;
  }
  hipKernelNodeParams np;
  std::memset(&np, 0, sizeof(np));
  np.func = const_cast<void*>(li.fn);
  np.gridDim = dim3((unsigned)li.grid);
  np.blockDim = dim3(qs::kBlock);
  np.sharedMemBytes = (unsigned)li.lds;
  np.kernelParams = args;   // (the runtime copies the arguments during the call)
  if (hipGraphKernelNodeSetParams(node, &np) != hipSuccess) { (void)hipGetLastError(); return false; }
  fuse_params<T>(h) = P;
  if (grow) {
    g.append(fo);
  } else {
    g.wrap();
    if (h->fuse_ring_steps == 0) h->ring[0] += 1;
    h->ring[1] += g.total - h->fuse_ring_steps;
    h->fuse_ring_steps = g.total;
  }
  // the node now names instance `kind`: it counts there, and no longer where it did
  if (h->fuse_kind >= 0) h->launches[h->fuse_kind] -= 1;
  h->launches[kind] += 1;
  h->fuse_kind = kind;
  return true;
}

// After a single-step synthetic-policy launch on a capturing stream: remember
// the kernel node it became, so that the next qs_step may join it.
template <class T> static void note_capture(qs_handle* h, const qs::Params<T>& P, const qs_step_out& o, hipStream_t st,
                                            const LaunchInfo& li) {
  const CaptureState c = capture_state(st);
  if (!c.active || c.ndeps != 1) return;
  hipGraphNodeType ty;
  hipKernelNodeParams np;
  if (hipGraphNodeGetType(c.deps[0], &ty) != hipSuccess || ty != hipGraphNodeTypeKernel ||
      hipGraphKernelNodeGetParams(c.deps[0], &np) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  if (np.func != li.fn) return;   // not the launch just made
  size_t sizes[qs::kFuseOuts];
  out_sizes(h, sizes);
  h->fuse.begin(sizes, to_outs(o), c.id, (void*)st, (void*)c.deps[0]);
  h->fuse_kind = -1;   // a single step so far
  h->fuse_ring_steps = 0;
  qs::ParamsMany<T>& F = fuse_params<T>(h);
  std::memset(&F, 0, sizeof(F));
  static_cast<qs::Params<T>&>(F) = P;
  F.io[0] = to_io<T>(o);
  F.nsteps = 1;
}

template <class T> static int step_impl(qs_handle* h, const float* actions, const qs_step_out& o, hipStream_t st) {
  // steps that may share a launch: synthetic policy, no search launch between two steps
  const bool fusable = h->fuse_depth > 1 && actions == nullptr && h->rq == nullptr;
  if (fusable && h->fuse.live && try_coalesce<T>(h, o, st)) return QS_OK;
  h->fuse.forget();
  qs::Params<T> P;
  single_step_params(h, P, actions, o);
  LaunchInfo li;
  const int rc = launch(h, P, st, &li);
  if (rc == QS_OK && fusable) note_capture<T>(h, P, o, st, li);
  return rc;
}

template <class T> static int step_many_impl(qs_handle* h, int n, const qs_step_out* outs, hipStream_t st) {
  const int depth = h->rq ? 1 : h->fuse_depth;   // the search launch sits between two steps of an env
  size_t sizes[qs::kFuseOuts];
  out_sizes(h, sizes);
  for (int j = 0; j < n;) {
    // the longest run of steps from j whose outputs are pairwise disjoint, up to the depth
    qs::FuseGroup g;
    g.begin(sizes, to_outs(outs[j]));
    while (j + g.count < n && g.can_append(to_outs(outs[j + g.count]), depth)) g.append(to_outs(outs[j + g.count]));
    qs::ParamsMany<T> P;
    std::memset(&P, 0, sizeof(P));
    single_step_params<T>(h, P, nullptr, outs[j]);
    int rc;
    if (g.count > 1) {
      P.nsteps = g.count;
      for (int k = 0; k < g.count; ++k) P.io[k] = to_io<T>(outs[j + k]);
      // then the steps that write the run's sets again in order, while the run is the hot shape's
      if (j + g.total < n && g.can_wrap(to_outs(outs[j + g.total]), depth, h->ring_max) && ring_eligible(h, P, st))
        while (j + g.total < n && g.can_wrap(to_outs(outs[j + g.total]), depth, h->ring_max)) g.wrap();
      if (g.total > g.count) {
        qs::ParamsRing<T> R;
        rc = launch_ring(h, P, g.total, st, R);
      } else {
        rc = launch_many(h, P, st);
      }
    } else {
      rc = launch<T>(h, P, st);
    }
    if (rc != QS_OK) return rc;
    j += g.total;
  }
  return QS_OK;
}

// qs_step_seq with actions: the longest runs of steps that may share a launch
// (step_fuse.h, SeqGroup), each run one launch of the FUSE = 2 instance; a run of
// one step is the single-step launch.
template <class T> static int step_seq_impl(qs_handle* h, int n, const float* const* actions, const qs_step_out* outs,
                                            hipStream_t st) {
  const int depth = seq_depth(h);
  size_t sizes[qs::kFuseOuts];
  out_sizes(h, sizes);
  const size_t act_bytes = sizes[6];   // N·A·4, as actions_out
  for (int j = 0; j < n;) {
    qs::SeqGroup g;
    g.begin(sizes, to_outs(outs[j]), actions[j], act_bytes);
    while (j + g.count() < n && g.can_append(to_outs(outs[j + g.count()]), actions[j + g.count()], depth))
      g.append(to_outs(outs[j + g.count()]), actions[j + g.count()]);
    const int cnt = g.count();
    int rc;
    if (cnt > 1) {
      qs::ParamsSeq<T> P;
      std::memset(&P, 0, sizeof(P));
      single_step_params<T>(h, P, nullptr, outs[j]);
      P.nsteps = cnt;
      for (int k = 0; k < cnt; ++k) {
        P.io[k] = to_io<T>(outs[j + k]);
        P.act[k] = actions[j + k];
      }
      rc = launch_kernel<T, 2>(h, P, st, nullptr, false);
    } else {
      qs::Params<T> P;
      single_step_params<T>(h, P, actions[j], outs[j]);
      rc = launch<T>(h, P, st);
    }
    if (rc != QS_OK) return rc;
    j += cnt;
  }
  return QS_OK;
}

// ---------------------------------------------------------------- branch rollouts
// Why a handle cannot score (nullptr: it can).
static const char* score_refusal(const qs_handle* h) {
  if (h->rq) return "this layout's reset draws can be rejected and the deferred search launch runs after each step";
  if (h->spec.task != QS_TASK_MULTIHOVER && h->spec.task != QS_TASK_SPIRAL)
    return "the multi-step kernels of the Flock / Meetup / LeaderFollower family round the env reward 1 ulp apart "
           "from the single step's";
  return nullptr;
}
// Steps of one qs_score launch (step_score.h).  The LDS figures are those of a
// launch whose workgroups need not share a CU (lds_plan at residency 1: the
// largest obs stage any launch of the handle gets), so the depth depends
// neither on C nor on QS_MAX_FUSED_STEPS.
static int score_depth(const qs_handle* h) {
  if (score_refusal(h)) return 0;
  int stage_rows = 0;
  size_t plan = 0;
  if (lds_plan(h->dims, envs_per_wave(h), 1, &stage_rows, &plan) != QS_OK) return 0;
  const size_t hist = (size_t)h->dims.hist_len * qs::kBlock * h->dims.act_dim * sizeof(float);
  const size_t image = fixed_ctrl_freq(h->spec) ? 0 : hist;
  return qs::score_depth(kSeqLdsMax, kLdsStatic + kLdsGrain, image, plan - hist, h->dims.act_dim);
}

// `who`: the entry point, qs_score, qs_score_agents, qs_track_score or qs_avoid_score; ret_agent: the latter
// three's extra output, or null; track / cost_agent: qs_track_score's spec (checked by the caller) and its output,
// or both null; avoid: qs_avoid_score's spec (checked by the caller; its track may be null), or null.
template <class T> static int score_impl(const char* who_c, qs_handle* h, int n, int C, const float* const* actions,
                                         const qs_step_out* outs, const qs_score_out* score, double* ret_agent,
                                         const qs_track_spec* track, double* cost_agent, const qs_avoid_spec* avoid,
                                         hipStream_t st) {
  const std::string who = std::string(who_c) + ": ";
  const qs_dims& d = h->dims;
  uint64_t bytes[qs::kScoreOuts], act_bytes = 0;
  const qs::ScoreShape shape{C, d.num_envs, d.num_drones, d.obs_dim, d.act_dim, d.precision};
  if (!qs::score_sizes(shape, bytes, &act_bytes) || !qs::score_fits(act_bytes))
    return fail(QS_E_INVALID, who + "C * num_envs * num_drones is too large for one launch (32-bit offsets)");
  qs::ScoreRanges ranges;
  bool any_out = false, room = true;
  const char* const names[qs::kScoreOuts] = {"obs", "reward", "terminated", "truncated", "terminal_obs", "reasons",
                                             "actions_out", "ret", "first_done"};
  auto add_out = [&](const void* p, int i) -> bool {   // false: too large to address
    if (!p) return true;
    any_out = true;
    if (!qs::score_fits(bytes[i])) return false;
    room = ranges.add(p, bytes[i], false) && room;
    return true;
  };
  for (int j = 0; j < n; ++j) {
    room = ranges.add(actions[j], act_bytes, true) && room;
    if (!outs) continue;
    const qs::FuseOuts fo = to_outs(outs[j]);
    for (int i = 0; i < qs::kFuseOuts; ++i)
      if (!add_out(fo.p[i], i))
        return fail(QS_E_INVALID, who + names[i] + " of C * num_envs envs is too large (32-bit offsets)");
  }
  if (score) {
    if (!add_out(score->ret, 7) || !add_out(score->first_done, 8))
      return fail(QS_E_INVALID, who + "C * num_envs is too large (32-bit offsets)");
  }
  if (ret_agent) {
    any_out = true;
    const uint64_t ab = qs::score_agent_bytes(shape);
    if (!qs::score_fits(ab))
      return fail(QS_E_INVALID, who + "ret_agent of C * num_envs * num_drones doubles is too large (32-bit offsets)");
    room = ranges.add(ret_agent, ab, false) && room;
  }
  if (cost_agent) {
    any_out = true;
    const uint64_t cb = qs::track_cost_bytes(C, d.num_envs, d.num_drones);
    if (!qs::score_fits(cb))
      return fail(QS_E_INVALID, who + "cost_agent of C * num_envs * num_drones doubles is too large (32-bit offsets)");
    // (held against every range by hand: ScoreRanges has room for qs_score_agents' ranges only)
    for (int i = 0; i < ranges.n; ++i)
      if (qs::avoid_ranges_meet((uintptr_t)cost_agent, cb, ranges.r[i].lo, ranges.r[i].hi))
        return fail(QS_E_INVALID, who + "cost_agent overlaps another output or an action buffer");
  }
  if (!any_out) return fail(QS_E_INVALID, who + "nothing to write (no output in outs[] and neither ret nor first_done)");
  if (!room || ranges.overlap())
    return fail(QS_E_INVALID, who + "an output overlaps another output or an action buffer");
  auto fill = [&](qs::ParamsScore<T>& P) {
    fill_params(h, P);
    P.mode = qs::MODE_STEP;
    P.E_src = d.num_envs;
    P.E = C * d.num_envs;          // the virtual envs; P.N stays the handle's agent count
    P.reset_queue = nullptr;       // (score_refusal: none)
    P.store_state = 0;             // nothing is stored to the handle, ever
    P.nsteps = n;
    for (int j = 0; j < n; ++j) {
      if (outs) P.io[j] = to_io<T>(outs[j]);
      P.act[j] = actions[j];
    }
    if (score) { P.ret = (double*)score->ret; P.first_done = score->first_done; }
    P.ret_agent = ret_agent;
  };
  auto fill_track = [&](qs::ParamsTrack<T>& P) {
    fill(P);
    P.ref = track->ref;
    P.base = track->base;
    P.L = track->L;
    for (int k = 0; k < qs::kTrackState; ++k) P.q[k] = track->q[k];
    for (int k = 0; k < qs::kTrackMaxAct; ++k) P.r[k] = k < d.act_dim ? track->r[k] : 0.0f;
    P.terminal = track->terminal;
    P.cost_agent = cost_agent;
  };
  if (avoid) {   // the FUSE = 6 instance: the tracking launch, or one without a reference, plus the avoidance terms
    static_assert(qs::kAvoidMaxRows == qs::kAvoidMaxObs, "the table's rows: avoid_sizes.h and step_kernel.h");
    qs::ParamsAvoid<T> P;
    std::memset(&P, 0, sizeof(P));
    if (track) {
      fill_track(P);
    } else {   // ref stays null: the kernel reads no reference and sums no tracking term
      fill(P);
      P.L = 1;
      P.cost_agent = cost_agent;
    }
    P.obstacles = avoid->M > 0 ? avoid->obstacles : nullptr;
    P.M = avoid->M;
    P.sep_radius = avoid->sep_radius;
    P.sep_weight = avoid->sep_weight;
    P.sep_z_scale = avoid->sep_z_scale;
    return launch_kernel<T, 6>(h, P, st, nullptr, false);
  }
  if (track) {   // the FUSE = 5 instance: the same launch plus the cost
    qs::ParamsTrack<T> P;
    std::memset(&P, 0, sizeof(P));
    fill_track(P);
    return launch_kernel<T, 5>(h, P, st, nullptr, false);
  }
  qs::ParamsScore<T> P;
  std::memset(&P, 0, sizeof(P));
  fill(P);
  return launch_kernel<T, 3>(h, P, st, nullptr, false);
}

// ---------------------------------------------------------------- branch sets
// The state of C · E virtual envs in one allocation (step_branch.h's six blocks),
// and a second one of the same size that qs_branch_select gathers into.
struct qs_branch {
  qs_handle* h = nullptr;
  int C = 0;
  qs::BranchSizes sz{};
  char* set = nullptr;      // the blocks; qs_branch_buffers' pointers lie in it
  char* shadow = nullptr;   // select's gather target, copied back whole
  int64_t steps = 0;        // advanced since the last fork
  bool forked = false;
  void* block(int i) const { return set + sz.offset[i]; }
};
enum { BR_AGENT = 0, BR_ENV = 1, BR_HIST = 2, BR_RET = 3, BR_FD = 4, BR_RET_AGENT = 5 };

// The six blocks as branch_move_kernel's segments: `src` / `dst` the allocations
// the blocks lie in (src = nullptr: the handle's own three state blocks, tiled,
// and zeros for the accumulators).
static qs::BranchMove branch_segments(const qs_branch* b, const char* src, char* dst, const int32_t* parent) {
  const qs_handle* h = b->h;
  const qs_dims& d = h->dims;
  const unsigned E = (unsigned)d.num_envs, D = (unsigned)d.num_drones, C = (unsigned)b->C;
  // bytes of one env's share of a row, and rows, per block
  const unsigned env_bytes[qs::kBranchBlocks] = {D * (unsigned)d.precision, (unsigned)qs::kEnvRec * 4u,
                                                 D * (unsigned)d.act_dim * 4u, 8u, 4u, D * 8u};
  const unsigned rows[qs::kBranchBlocks] = {QS_AGENT_FIELDS, 1u, (unsigned)d.hist_len, 1u, 1u, 1u};
  const void* const from_handle[qs::kBranchBlocks] = {h->st, h->env, h->hist, nullptr, nullptr, nullptr};
  qs::BranchMove m;
  std::memset(&m, 0, sizeof(m));
  m.parent = parent;
  m.C = C;
  m.E = E;
  for (int i = 0; i < qs::kBranchBlocks; ++i) {
    qs::BranchSeg& g = m.seg[i];
    g.unit = env_bytes[i] % 16u == 0 ? 16u : 4u;   // (every block starts 256-byte aligned; rows are whole envs)
    g.per_env = env_bytes[i] / g.unit;
    g.row = E * g.per_env;
    g.rows = rows[i];
    g.cand = C;
    g.src_cand = src ? C : 1u;
    g.src = src ? static_cast<const void*>(src + b->sz.offset[i]) : from_handle[i];
    g.dst = dst + b->sz.offset[i];
  }
  return m;
}
static int branch_move(const qs_branch* b, const qs::BranchMove& m, hipStream_t st) {
  uint64_t most = 0;
  for (int i = 0; i < qs::kBranchBlocks; ++i) most = std::max<uint64_t>(most, b->sz.bytes[i] / m.seg[i].unit);
  const unsigned gx = (unsigned)std::min<uint64_t>(std::max<uint64_t>((most + 255) / 256, 1), 2048);
  hipLaunchKernelGGL(qs::branch_move_kernel, dim3(gx, qs::kBranchBlocks), dim3(256), 0, st, m);
  HIP_TRY(hipGetLastError());
  return QS_OK;
}

template <class T> static int branch_advance_impl(qs_branch* b, int n, const float* const* actions, const qs_step_out* outs,
                                                  hipStream_t st) {
  const std::string who = "qs_branch_advance: ";
  qs_handle* h = b->h;
  const qs_dims& d = h->dims;
  uint64_t bytes[qs::kScoreOuts], act_bytes = 0;
  const qs::ScoreShape shape{b->C, d.num_envs, d.num_drones, d.obs_dim, d.act_dim, d.precision};
  if (!qs::score_sizes(shape, bytes, &act_bytes) || !qs::score_fits(act_bytes))
    return fail(QS_E_INVALID, who + "C * num_envs * num_drones is too large for one launch (32-bit offsets)");
  qs::ScoreRanges ranges;
  bool room = true;
  const char* const names[qs::kFuseOuts] = {"obs", "reward", "terminated", "truncated", "terminal_obs", "reasons", "actions_out"};
  for (int j = 0; j < n; ++j) {
    room = ranges.add(actions[j], act_bytes, true) && room;
    if (!outs) continue;
    const qs::FuseOuts fo = to_outs(outs[j]);
    for (int i = 0; i < qs::kFuseOuts; ++i) {
      if (!fo.p[i]) continue;
      if (!qs::score_fits(bytes[i]))
        return fail(QS_E_INVALID, who + names[i] + " of C * num_envs envs is too large (32-bit offsets)");
      room = ranges.add(fo.p[i], bytes[i], false) && room;
    }
  }
  room = ranges.add(b->set, b->sz.total, false) && room;   // the set itself is written: nothing named may lie in it
  if (!room || ranges.overlap())
    return fail(QS_E_INVALID, who + "an output overlaps another output, an action buffer or the branch set");
  qs::ParamsBranch<T> P;
  std::memset(&P, 0, sizeof(P));
  fill_params(h, P);
  P.mode = qs::MODE_STEP;
  P.E_src = d.num_envs;
  P.E = (int)b->sz.V;
  P.N = (int)b->sz.N;
  P.st = (T*)b->block(BR_AGENT);
  P.env = (int32_t*)b->block(BR_ENV);
  P.hist = (float*)b->block(BR_HIST);
  P.log = nullptr;               // a branch logs no episodes and raises no reset error
  P.err = nullptr;
  P.reset_queue = nullptr;       // (score_refusal: none)
  P.reset_pre = nullptr;
  P.store_state = 1;
  P.nsteps = n;
  for (int j = 0; j < n; ++j) {
    if (outs) P.io[j] = to_io<T>(outs[j]);
    P.act[j] = actions[j];
  }
  P.ret = (double*)b->block(BR_RET);
  P.first_done = (int32_t*)b->block(BR_FD);
  P.ret_agent = (double*)b->block(BR_RET_AGENT);
  P.t0 = (int)b->steps;
  const int rc = launch_kernel<T, 4>(h, P, st, nullptr, false);
  if (rc == QS_OK) b->steps += n;
  return rc;
}

// planner.hip's view of a handle (planner_link.h).
namespace qs {
void handle_info(const qs_handle* h, HandleInfo* out) {
  out->device = h->device;
  out->env_offset = h->spec.env_offset;
  out->reset_done = h->reset_done;
}
int set_last_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace qs

extern "C" {

const char* qs_last_error(void) { return g_err.c_str(); }
int qs_abi_version(void) { return QS_ABI_VERSION; }

// Default fusion depth of the synthetic-policy rollout (QS_MAX_FUSED_STEPS
// overrides it): the fastest of 1 / 8 / 16 / 24 / 32 on the C3 bench (profiles/step_trim_ab.json).
static constexpr int kDefaultFusedSteps = 32;

int qs_create(const qs_spec* spec, int device, qs_handle** out) {
  if (!spec || !out) return fail(QS_E_INVALID, "qs_create: null argument");
  const qs_spec& s = *spec;
  if (s.task < QS_TASK_MULTIHOVER || s.task > QS_TASK_LEADERFOLLOWER) return fail(QS_E_INVALID, "qs_create: bad task");
  if (s.num_drones < 1 || s.num_drones > 64) return fail(QS_E_INVALID, "qs_create: num_drones must be in 1..64");
  if (s.num_envs < 1) return fail(QS_E_INVALID, "qs_create: num_envs must be >= 1");
  if (s.physics != QS_PHYS_DYN && s.physics != QS_PHYS_PYB) return fail(QS_E_INVALID, "qs_create: bad physics");
  if (s.aux_forces & ~7u) return fail(QS_E_INVALID, "qs_create: bad aux_forces");
  if (s.flags & ~(QS_FLAG_NO_AUTORESET | QS_FLAG_INKERNEL_RESET_SEARCH | QS_FLAG_CF2P))
    return fail(QS_E_INVALID, "qs_create: bad flags");
  if (s.pyb_freq <= 0 || s.ctrl_freq <= 0 || s.pyb_freq % s.ctrl_freq)
    return fail(QS_E_INVALID, "qs_create: pyb_freq is not divisible by env_freq");  // BaseAviary.py:79-80
  if (s.ctrl_freq < 2) return fail(QS_E_INVALID, "qs_create: ctrl_freq must be >= 2 (action history length ctrl_freq//2)");
  if (s.precision != 4 && s.precision != 8) return fail(QS_E_INVALID, "qs_create: precision must be 4 or 8");
  if (check_consts() != QS_OK) return QS_E_INVALID;
  if (s.task == QS_TASK_MULTIHOVER && !s.initial_xyzs && s.num_drones >= 6)
    return fail(QS_E_INVALID, "qs_create: MultiHover reset with the default diagonal layout cannot complete for "
                              "D >= 6 (SURVEY §7 hard-2); pass initial_xyzs");
  int A;
  switch (s.act_type) {
    case QS_ACT_RPM: case QS_ACT_VEL: A = 4; break;
    case QS_ACT_PID: A = 3; break;
    case QS_ACT_ONE_D_RPM: case QS_ACT_ONE_D_PID: A = 1; break;
    default: return fail(QS_E_INVALID, "qs_create: bad act_type");
  }
  {
    // The kernels address every buffer through 32-bit buffer-resource ranges and
    // offsets (step_kernel.h: state, history, obs rows, env records): refuse a
    // shard whose largest buffer would not fit below 2^31 bytes instead of
    // letting the offsets wrap.  (C3 at 16 384 envs uses 15 MB.)
    const int64_t Nn = (int64_t)s.num_envs * s.num_drones;
    const int64_t H = s.ctrl_freq / 2;
    const int64_t O = 12 + H * A + (s.task == QS_TASK_SPIRAL ? 11 : 0);
    const int64_t biggest = std::max({(int64_t)QS_AGENT_FIELDS * Nn * s.precision, H * Nn * A * 4, Nn * O * 4,
                                      (int64_t)qs::kEnvRec * s.num_envs * 4});
    if (biggest >= (int64_t(1) << 31))
      return fail(QS_E_INVALID, "qs_create: num_envs * num_drones too large for one handle (a state buffer would "
                                "exceed 2^31 bytes); shard the envs over more handles");
  }
  HIP_TRY(hipSetDevice(device));
  auto* h = new (std::nothrow) qs_handle();
  if (!h) return fail(QS_E_NOMEM, "qs_create: host allocation failed");
  h->fuse_depth = kDefaultFusedSteps;
  if (const char* v = getenv("QS_MAX_FUSED_STEPS")) {   // read once, here
    char* end = nullptr;
    const long k = std::strtol(v, &end, 10);
    if (end != v) h->fuse_depth = (int)std::min<long>(std::max<long>(k, 1), qs::kMaxFuse);
  }
  if (const char* v = getenv("QS_WAVE_REDUCE")) h->wave_reduce = std::strtol(v, nullptr, 10) != 0;   // read once, here
  if (const char* v = getenv("QS_HOT_SHAPE")) h->hot_shape = std::strtol(v, nullptr, 10) != 0;       // read once, here
  if (const char* v = getenv("QS_RING_LAUNCH")) h->ring_launch = std::strtol(v, nullptr, 10) != 0;   // read once, here
  if (const char* v = getenv("QS_RING_MAX_STEPS")) {                                                 // read once, here
    char* end = nullptr;
    const long k = std::strtol(v, &end, 10);
    if (end != v) h->ring_max = (int)std::min<long>(std::max<long>(k, 1), qs::kRingMaxSteps);
  }
  h->spec = s;
  h->spec.initial_xyzs = nullptr;
  h->device = device;
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0)
      h->num_cu = cu;
  }
  qs_dims& d = h->dims;
  d.num_envs = s.num_envs; d.num_drones = s.num_drones; d.num_agents = s.num_envs * s.num_drones;
  d.act_dim = A; d.hist_len = s.ctrl_freq / 2; d.substeps = s.pyb_freq / s.ctrl_freq;
  d.obs_dim = 12 + d.hist_len * A + (s.task == QS_TASK_SPIRAL ? 11 : 0);
  d.precision = s.precision; d.agent_fields = QS_AGENT_FIELDS; d.env_fields = QS_ENV_FIELDS;
  {
    int rows; size_t bytes;
    if (lds_plan(d, qs::kBlock / s.num_drones, 1, &rows, &bytes) != QS_OK) {
      delete h;
      return fail(QS_E_INVALID, "qs_create: action history (ctrl_freq // 2 entries) does not fit in LDS");
    }
  }
  // initial layout (BaseAviary.py:194-197 / SpiralAviary.py:47-53)
  const HostConsts C;
  h->orig_host.resize(3 * s.num_drones);
  for (int i = 0; i < s.num_drones; ++i) {
    double xyz[3];
    if (s.initial_xyzs) { for (int k = 0; k < 3; ++k) xyz[k] = s.initial_xyzs[i * 3 + k]; }
    else if (s.task == QS_TASK_SPIRAL) {
      xyz[0] = s.spiral_radius * std::cos(2 * M_PI * i / s.num_drones);
      xyz[1] = s.spiral_radius * std::sin(2 * M_PI * i / s.num_drones);
      xyz[2] = 0.3;
    } else {
      xyz[0] = i * 4 * C.L; xyz[1] = i * 4 * C.L; xyz[2] = C.COLL_H / 2 - C.COLL_Z_OFF + .1;
    }
    for (int k = 0; k < 3; ++k) h->orig_host[i * 3 + k] = xyz[k];
  }
  // MultiHover reset draws are rejected when two drones come within 0.5 m
  // (MH:96-101).  The U(±0.25) noise moves a pair by < 0.5 per axis, so a layout
  // whose every pair is >= 1 m apart in x or y never rejects (the bench's grid);
  // otherwise (the reference's default diagonal layout) rejected envs are queued
  // for reset_search_kernel instead of being searched inside the step.
  bool can_reject = false;
  for (int i = 0; i < s.num_drones; ++i)
    for (int j = i + 1; j < s.num_drones; ++j)
      if (std::fabs(h->orig_host[i * 3] - h->orig_host[j * 3]) < 1.0 &&
          std::fabs(h->orig_host[i * 3 + 1] - h->orig_host[j * 3 + 1]) < 1.0)
        can_reject = true;
  // (z is clipped to [0.1, 1], so MH:96's z < 0.1 test never rejects either)
  h->reject_free = s.task == QS_TASK_MULTIHOVER && !can_reject;
  const bool may_reject = s.task == QS_TASK_MULTIHOVER && s.num_drones <= qs::kResetMaxD && can_reject;
  const size_t rs = (size_t)s.precision;
  const size_t N = d.num_agents;
  // per-env episode rings: at least 8 slots each, 65 536 records in all for small batches
  h->log_per_env = (int)std::max<int64_t>(8, ((int64_t)1 << 16) / std::max(1, s.num_envs));
  auto cleanup = [&]() { qs_destroy(h); };
  hipError_t e1 = hipMalloc(&h->st, rs * QS_AGENT_FIELDS * N);
  hipError_t e2 = hipMalloc((void**)&h->env, sizeof(int32_t) * qs::kEnvRec * s.num_envs);
  hipError_t e3 = hipMalloc((void**)&h->hist, sizeof(float) * d.hist_len * N * A);
  hipError_t e5 = hipMalloc(&h->orig, rs * 3 * s.num_drones);
  hipError_t e6 = hipMalloc((void**)&h->log, sizeof(qs_episode_rec) * h->log_per_env * (size_t)s.num_envs);
  hipError_t e7 = hipSuccess;
  hipError_t e8 = hipMalloc((void**)&h->err, sizeof(int));
  if (e1 || e2 || e3 || e5 || e6 || e7 || e8) { cleanup(); return fail(QS_E_NOMEM, "qs_create: hipMalloc failed"); }
  if (may_reject && !(s.flags & QS_FLAG_INKERNEL_RESET_SEARCH)) {
    // header line {count, envs written}, then one 128-B record per slot
    // (initialised when the step kernel queues an env; qs::reset_search_kernel)
    const size_t qn = (size_t)qs::kRqLine * (1 + (size_t)s.num_envs);
    if (hipMalloc((void**)&h->rq, sizeof(int) * qn) != hipSuccess) { cleanup(); return fail(QS_E_NOMEM, "qs_create: hipMalloc failed"); }
    if (hipMalloc((void**)&h->rpre, sizeof(int32_t) * (size_t)s.num_envs) != hipSuccess) {
      cleanup(); return fail(QS_E_NOMEM, "qs_create: hipMalloc failed");
    }
    if (hipMemset(h->rq, 0, sizeof(int) * qn) ||
        hipMemset(h->rpre, 0, sizeof(int32_t) * (size_t)s.num_envs)) {
      cleanup(); return fail(QS_E_HIP, "qs_create: memset");
    }
  }
  if (s.precision == 8) {
    if (hipMemcpy(h->orig, h->orig_host.data(), 8 * 3 * s.num_drones, hipMemcpyHostToDevice)) { cleanup(); return fail(QS_E_HIP, "qs_create: copy"); }
  } else {
    std::vector<float> of(h->orig_host.begin(), h->orig_host.end());
    if (hipMemcpy(h->orig, of.data(), 4 * 3 * s.num_drones, hipMemcpyHostToDevice)) { cleanup(); return fail(QS_E_HIP, "qs_create: copy"); }
  }
  if (hipMemset(h->st, 0, rs * QS_AGENT_FIELDS * N) || hipMemset(h->env, 0, sizeof(int32_t) * qs::kEnvRec * s.num_envs) ||
      hipMemset(h->hist, 0, sizeof(float) * d.hist_len * N * A) ||
      hipMemset(h->err, 0, sizeof(int))) {
    cleanup(); return fail(QS_E_HIP, "qs_create: memset");
  }
#ifdef QS_STAMPS_BUILD
  if (getenv("QS_STAMPS")) {   // dev-only phase timestamps
    const int grid = (s.num_envs + qs::kBlock / s.num_drones - 1) / (qs::kBlock / s.num_drones);
    if (hipMalloc((void**)&h->stamps, sizeof(unsigned long long) * 8 * grid) == hipSuccess)
      hipMemset(h->stamps, 0, sizeof(unsigned long long) * 8 * grid);
  }
#endif
  *out = h;
  return QS_OK;
}

// dev-only: copy the per-wave phase timestamps (8 per workgroup) to host.
extern "C" int qs_debug_stamps(qs_handle* h, unsigned long long* host, int64_t n) {
  if (!h || !h->stamps) return fail(QS_E_STATE, "QS_STAMPS not enabled");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, h->stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return QS_OK;
}

int qs_destroy(qs_handle* h) {
  if (!h) return QS_OK;
  (void)hipSetDevice(h->device);   // teardown: best effort, nothing to report to
  void* ptrs[] = {h->st, h->env, h->hist, h->orig, h->log, h->err, h->stamps, h->rq, h->rpre, h->logw, h->log_sel};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  delete h;
  return QS_OK;
}

int qs_ring_counts(const qs_handle* h, int64_t* launches, int64_t* steps) {
  if (!h || !launches || !steps) return fail(QS_E_INVALID, "qs_ring_counts: null argument");
  *launches = h->ring[0];
  *steps = h->ring[1];
  return QS_OK;
}

int qs_launch_counts(const qs_handle* h, int64_t out[2]) {
  if (!h || !out) return fail(QS_E_INVALID, "qs_launch_counts: null argument");
  out[0] = h->launches[0];
  out[1] = h->launches[1];
  return QS_OK;
}

int qs_get_dims(const qs_handle* h, qs_dims* out) {
  if (!h || !out) return fail(QS_E_INVALID, "qs_get_dims: null argument");
  *out = h->dims;
  return QS_OK;
}

int qs_reset(qs_handle* h, uint64_t seed, float* obs, void* stream) {
  if (!h) return fail(QS_E_INVALID, "qs_reset: null handle");
  hipStream_t st = (hipStream_t)stream;
  h->fuse.forget();
  const qs_dims& d = h->dims;
  const size_t N = d.num_agents, rs = d.precision;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemsetAsync(h->st, 0, rs * QS_AGENT_FIELDS * N, st));
  HIP_TRY(hipMemsetAsync(h->env, 0, sizeof(int32_t) * qs::kEnvRec * d.num_envs, st));
  HIP_TRY(hipMemsetAsync(h->hist, 0, sizeof(float) * d.hist_len * N * d.act_dim, st));
  HIP_TRY(hipMemsetAsync(h->err, 0, sizeof(int), st));
  // the precomputed reset searches belong to the old (seed, episode) tags: restart
  // them, or a queued search would skip the new episode's first chunks (MH:83-102
  // takes the FIRST accepted try)
  if (h->rpre) HIP_TRY(hipMemsetAsync(h->rpre, 0, sizeof(int32_t) * d.num_envs, st));
  h->seed = seed;
  int rc;
  if (d.precision == 8) {
    qs::Params<double> P; fill_params(h, P); P.mode = qs::MODE_RESET_ALL; P.obs = obs;
    rc = launch(h, P, st);
  } else {
    qs::Params<float> P; fill_params(h, P); P.mode = qs::MODE_RESET_ALL; P.obs = obs;
    rc = launch(h, P, st);
  }
  if (rc == QS_OK) h->reset_done = true;
  return rc;
}

int qs_reset_envs(qs_handle* h, const uint8_t* mask, float* obs, void* stream) {
  if (!h) return fail(QS_E_INVALID, "qs_reset_envs: null handle");
  if (!h->reset_done) return fail(QS_E_STATE, "qs_reset_envs: call qs_reset first");
  hipStream_t st = (hipStream_t)stream;
  h->fuse.forget();
  if (h->dims.precision == 8) {
    qs::Params<double> P; fill_params(h, P); P.mode = qs::MODE_RESET_MASK; P.reset_mask = mask; P.obs = obs;
    return launch(h, P, st);
  }
  qs::Params<float> P; fill_params(h, P); P.mode = qs::MODE_RESET_MASK; P.reset_mask = mask; P.obs = obs;
  return launch(h, P, st);
}

int qs_step(qs_handle* h, const float* actions, const qs_step_out* out, void* stream) {
  if (!h) return fail(QS_E_INVALID, "qs_step: null handle");
  if (!h->reset_done) return fail(QS_E_STATE, "qs_step: call qs_reset first");
  hipStream_t st = (hipStream_t)stream;
  qs_step_out o{};
  if (out) o = *out;
  if (h->dims.precision == 8) return step_impl<double>(h, actions, o, st);
  return step_impl<float>(h, actions, o, st);
}

int qs_step_many(qs_handle* h, int n, const qs_step_out* outs, void* stream) {
  if (!h) return fail(QS_E_INVALID, "qs_step_many: null handle");
  if (n < 0 || (n > 0 && !outs)) return fail(QS_E_INVALID, "qs_step_many: bad argument");
  if (!h->reset_done) return fail(QS_E_STATE, "qs_step_many: call qs_reset first");
  h->fuse.forget();
  hipStream_t st = (hipStream_t)stream;
  if (h->dims.precision == 8) return step_many_impl<double>(h, n, outs, st);
  return step_many_impl<float>(h, n, outs, st);
}

int qs_step_seq(qs_handle* h, int n, const float* const* actions, const qs_step_out* outs, void* stream) {
  if (!h) return fail(QS_E_INVALID, "qs_step_seq: null handle");
  if (n < 0 || (n > 0 && !outs)) return fail(QS_E_INVALID, "qs_step_seq: bad argument");
  if (!h->reset_done) return fail(QS_E_STATE, "qs_step_seq: call qs_reset first");
  if (actions) {
    for (int j = 0; j < n; ++j)
      if (!actions[j])
        return fail(QS_E_INVALID, "qs_step_seq: actions[" + std::to_string(j) + "] is null (every step reads its "
                                  "actions or none does: pass actions = NULL for the random policy)");
  }
  h->fuse.forget();
  hipStream_t st = (hipStream_t)stream;
  if (!actions) {
    if (h->dims.precision == 8) return step_many_impl<double>(h, n, outs, st);
    return step_many_impl<float>(h, n, outs, st);
  }
  if (h->dims.precision == 8) return step_seq_impl<double>(h, n, actions, outs, st);
  return step_seq_impl<float>(h, n, actions, outs, st);
}

int qs_score_depth(const qs_handle* h) { return h ? score_depth(h) : 0; }

// Why a tracking spec is refused against handle h (track_sizes.h), as the message after the entry point's name.
static const char* track_refusal_text(const qs_handle* h, const qs_track_spec* s) {
  qs::TrackSpecShape v;
  v.ref = (uintptr_t)s->ref;
  v.L = s->L;
  for (int k = 0; k < qs::kTrackState; ++k) v.q[k] = s->q[k];
  for (int k = 0; k < qs::kTrackMaxAct; ++k) v.r[k] = s->r[k];
  v.terminal = s->terminal;
  v.reward_scale = s->reward_scale;
  switch (qs::track_refusal(v, h->dims.num_envs, h->dims.num_drones, h->dims.act_dim)) {
    case qs::kTrackRefNull: return "ref is null";
    case qs::kTrackRefAlign: return "ref must be 16-byte aligned";
    case qs::kTrackRows: return "L must be >= 1";
    case qs::kTrackQ: return "q[0 .. 11] must be finite and >= 0";
    case qs::kTrackR: return "r[a] must be finite and >= 0 for each action component";
    case qs::kTrackTerminal: return "terminal must be finite and >= 0";
    case qs::kTrackScale: return "reward_scale must be finite";
    case qs::kTrackOffsets: return "L * num_envs * num_drones * 48 bytes of ref are past the 32-bit offsets";
    default: return nullptr;
  }
}

// Why an avoidance spec is refused (avoid_sizes.h), as the message after the entry point's name.
static const char* avoid_refusal_text(const qs_avoid_spec* s) {
  const qs::AvoidSpecShape v{(uintptr_t)s->obstacles, s->M, s->sep_radius, s->sep_weight, s->sep_z_scale};
  return qs::avoid_refusal_text(qs::avoid_refusal(v));
}

// qs_score, qs_score_agents (ret_agent null: the same call under the other name), qs_track_score
// (tracking: spec and cost_agent must be there) and qs_avoid_score (avoiding: avoid and cost_agent must be
// there, track may be null).
static int score_entry(const char* who_c, qs_handle* h, int n, int C, const float* const* actions, const qs_step_out* outs,
                       const qs_score_out* score, double* ret_agent, void* stream, bool tracking = false,
                       const qs_track_spec* track = nullptr, double* cost_agent = nullptr, bool avoiding = false,
                       const qs_avoid_spec* avoid = nullptr) {
  const std::string who = std::string(who_c) + ": ";
  if (!h) return fail(QS_E_INVALID, who + "null handle");
  if (tracking) {
    if (!track) return fail(QS_E_INVALID, who + "spec is null");
    if (!cost_agent) return fail(QS_E_INVALID, who + "cost_agent is null");
  }
  if (avoiding) {
    if (!avoid) return fail(QS_E_INVALID, who + "avoid is null");
    if (!cost_agent) return fail(QS_E_INVALID, who + "cost_agent is null");
    tracking = track != nullptr;
  }
  if (const char* why = score_refusal(h)) return fail(QS_E_INVALID, who + "this handle cannot score: " + why);
  const int depth = score_depth(h);
  if (depth < 1) return fail(QS_E_INVALID, who + "this handle cannot score: no step's action rows fit in LDS");
  if (C < 1) return fail(QS_E_INVALID, who + "C must be >= 1");
  if (n < 1 || n > depth)
    return fail(QS_E_INVALID, who + "n = " + std::to_string(n) + " is outside 1 .. qs_score_depth = " +
                                  std::to_string(depth) + " (longer horizons are not cut into several launches)");
  if (!actions) return fail(QS_E_INVALID, who + "actions is null");
  for (int j = 0; j < n; ++j)
    if (!actions[j]) return fail(QS_E_INVALID, who + "actions[" + std::to_string(j) + "] is null");
  if (tracking)
    if (const char* why = track_refusal_text(h, track)) return fail(QS_E_INVALID, who + why);
  if (avoiding)
    if (const char* why = avoid_refusal_text(avoid)) return fail(QS_E_INVALID, who + why);
  if (!h->reset_done) return fail(QS_E_STATE, who + "call qs_reset first");
  h->fuse.forget();
  hipStream_t st = (hipStream_t)stream;
  if (h->dims.precision == 8)
    return score_impl<double>(who_c, h, n, C, actions, outs, score, ret_agent, track, cost_agent, avoid, st);
  return score_impl<float>(who_c, h, n, C, actions, outs, score, ret_agent, track, cost_agent, avoid, st);
}

int qs_avoid_score(qs_handle* h, int n, int C, const float* const* actions, const qs_step_out* outs,
                   const qs_score_out* score, double* ret_agent, const qs_track_spec* track, const qs_avoid_spec* avoid,
                   double* cost_agent, void* stream) {
  return score_entry("qs_avoid_score", h, n, C, actions, outs, score, ret_agent, stream, false, track, cost_agent, true,
                     avoid);
}

int qs_track_score(qs_handle* h, int n, int C, const float* const* actions, const qs_step_out* outs,
                   const qs_score_out* score, double* ret_agent, const qs_track_spec* spec, double* cost_agent,
                   void* stream) {
  return score_entry("qs_track_score", h, n, C, actions, outs, score, ret_agent, stream, true, spec, cost_agent);
}

int qs_score(qs_handle* h, int n, int C, const float* const* actions, const qs_step_out* outs, const qs_score_out* score,
             void* stream) {
  return score_entry("qs_score", h, n, C, actions, outs, score, nullptr, stream);
}

int qs_score_agents(qs_handle* h, int n, int C, const float* const* actions, const qs_step_out* outs,
                    const qs_score_out* score, double* ret_agent, void* stream) {
  return score_entry("qs_score_agents", h, n, C, actions, outs, score, ret_agent, stream);
}

// qs_state_io's view of the per-env records: counters as [QS_ENV_FIELDS][E]
// int32 (counters = true) or the episode returns as [E] f64.
// Written counters (the episode number among them) void the env's precomputed
// reset search: word 7 and its chunk counter start over.
__global__ void env_io_kernel(int32_t* rec, void* ext, int E, bool counters, bool to_rec, int32_t* pre) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int32_t* r = rec + (size_t)e * qs::kEnvRec;
  if (counters) {
    int32_t* x = (int32_t*)ext;
    for (int f = 0; f < QS_ENV_FIELDS; ++f) {
      if (to_rec) r[f] = x[(size_t)f * E + e];
      else x[(size_t)f * E + e] = r[f];
    }
    if (to_rec) {
      r[qs::kEnvPreWord] = 0;
      if (pre) pre[e] = 0;
    }
  } else {
    double* x = (double*)ext;
    double* rr = reinterpret_cast<double*>(r + qs::kEnvRetWord);
    if (to_rec) *rr = x[e];
    else x[e] = *rr;
  }
}

int qs_state_io(qs_handle* h, int block, void* buf, int dir, void* stream) {
  if (!h || !buf) return fail(QS_E_INVALID, "qs_state_io: null argument");
  hipStream_t st = (hipStream_t)stream;
  h->fuse.forget();
  const qs_dims& d = h->dims;
  void* src = nullptr;
  size_t bytes = 0;
  switch (block) {
    case QS_STATE_AGENT: src = h->st; bytes = (size_t)d.precision * QS_AGENT_FIELDS * d.num_agents; break;
    case QS_STATE_ENV:
    case QS_STATE_EP_RETURN: {   // the external layouts [4][E] int32 / [E] f64, from the records
      HIP_TRY(hipSetDevice(h->device));
      const int E = d.num_envs;
      env_io_kernel<<<(E + 255) / 256, 256, 0, st>>>(h->env, buf, E, block == QS_STATE_ENV, dir != 0, h->rpre);
      HIP_TRY(hipGetLastError());
      if (dir) h->reset_done = true;
      return QS_OK;
    }
    case QS_STATE_HISTORY: src = h->hist; bytes = sizeof(float) * d.hist_len * d.num_agents * d.act_dim; break;
    default: return fail(QS_E_INVALID, "qs_state_io: bad block");
  }
  HIP_TRY(hipSetDevice(h->device));
  if (dir) HIP_TRY(hipMemcpyAsync(src, buf, bytes, hipMemcpyDeviceToDevice, st));
  else HIP_TRY(hipMemcpyAsync(buf, src, bytes, hipMemcpyDeviceToDevice, st));
  if (dir) h->reset_done = true;
  return QS_OK;
}

// ---- branch sets (include/quadswarm.h)
int qs_branch_create(qs_handle* h, int C, qs_branch** out) {
  const std::string who = "qs_branch_create: ";
  if (!h || !out) return fail(QS_E_INVALID, who + "null argument");
  if (const char* why = score_refusal(h)) return fail(QS_E_INVALID, who + "this handle cannot score: " + why);
  if (score_depth(h) < 1) return fail(QS_E_INVALID, who + "this handle cannot score: no step's action rows fit in LDS");
  if (C < 1) return fail(QS_E_INVALID, who + "C must be >= 1");
  const qs_dims& d = h->dims;
  qs::BranchSizes sz;
  if (!qs::branch_sizes(qs::BranchShape{C, d.num_envs, d.num_drones, d.hist_len, d.act_dim, QS_AGENT_FIELDS, d.precision}, &sz))
    return fail(QS_E_INVALID, who + "a state block of C * num_envs * num_drones agents is too large (32-bit offsets)");
  HIP_TRY(hipSetDevice(h->device));
  auto* b = new (std::nothrow) qs_branch();
  if (!b) return fail(QS_E_NOMEM, who + "host allocation failed");
  b->h = h;
  b->C = C;
  b->sz = sz;
  if (hipMalloc((void**)&b->set, sz.total) != hipSuccess || hipMalloc((void**)&b->shadow, sz.total) != hipSuccess ||
      hipMemset(b->set, 0, sz.total) != hipSuccess || hipMemset(b->shadow, 0, sz.total) != hipSuccess) {
    (void)hipGetLastError();
    qs_branch_destroy(b);
    return fail(QS_E_NOMEM, who + "hipMalloc failed");
  }
  *out = b;
  return QS_OK;
}

int qs_branch_destroy(qs_branch* b) {
  if (!b) return QS_OK;
  (void)hipSetDevice(b->h->device);   // teardown: best effort, nothing to report to
  if (b->set) (void)hipFree(b->set);
  if (b->shadow) (void)hipFree(b->shadow);
  delete b;
  return QS_OK;
}

int qs_branch_buffers(const qs_branch* b, qs_branch_bufs* out) {
  if (!b || !out) return fail(QS_E_INVALID, "qs_branch_buffers: null argument");
  out->ret = (double*)b->block(BR_RET);
  out->first_done = (int32_t*)b->block(BR_FD);
  out->ret_agent = (double*)b->block(BR_RET_AGENT);
  return QS_OK;
}

int qs_branch_steps(const qs_branch* b, int64_t* out) {
  if (!b || !out) return fail(QS_E_INVALID, "qs_branch_steps: null argument");
  *out = b->steps;
  return QS_OK;
}

int qs_branch_fork(qs_branch* b, void* stream) {
  if (!b) return fail(QS_E_INVALID, "qs_branch_fork: null branch set");
  if (!b->h->reset_done) return fail(QS_E_STATE, "qs_branch_fork: call qs_reset first");
  b->h->fuse.forget();
  const int rc = branch_move(b, branch_segments(b, nullptr, b->set, nullptr), (hipStream_t)stream);
  if (rc != QS_OK) return rc;
  b->steps = 0;
  b->forked = true;
  return QS_OK;
}

int qs_branch_advance(qs_branch* b, int n, const float* const* actions, const qs_step_out* outs, void* stream) {
  const std::string who = "qs_branch_advance: ";
  if (!b) return fail(QS_E_INVALID, who + "null branch set");
  qs_handle* h = b->h;
  const int depth = score_depth(h);
  if (n < 1 || n > depth)
    return fail(QS_E_INVALID, who + "n = " + std::to_string(n) + " is outside 1 .. qs_score_depth = " + std::to_string(depth) +
                                  " (call it again to go on: the branch set keeps the state)");
  if (!actions) return fail(QS_E_INVALID, who + "actions is null");
  for (int j = 0; j < n; ++j)
    if (!actions[j]) return fail(QS_E_INVALID, who + "actions[" + std::to_string(j) + "] is null");
  if (!b->forked) return fail(QS_E_STATE, who + "call qs_branch_fork first");
  if (!qs::branch_steps_fit(b->steps, n))
    return fail(QS_E_INVALID, who + "first_done could not hold the step index: fork again");
  h->fuse.forget();
  hipStream_t st = (hipStream_t)stream;
  if (h->dims.precision == 8) return branch_advance_impl<double>(b, n, actions, outs, st);
  return branch_advance_impl<float>(b, n, actions, outs, st);
}

int qs_branch_select(qs_branch* b, const int32_t* parent, void* stream) {
  if (!b || !parent) return fail(QS_E_INVALID, "qs_branch_select: null argument");
  if (!b->forked) return fail(QS_E_STATE, "qs_branch_select: call qs_branch_fork first");
  b->h->fuse.forget();
  hipStream_t st = (hipStream_t)stream;
  // every candidate reads the old set: gather into the shadow, then copy it back whole
  // (the set's pointers stay what they were, on every replay of a captured call too)
  const int rc = branch_move(b, branch_segments(b, b->set, b->shadow, parent), st);
  if (rc != QS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(b->set, b->shadow, b->sz.total, hipMemcpyDeviceToDevice, st));
  return QS_OK;
}

int qs_branch_state(qs_branch* b, int block, void* buf, void* stream) {
  if (!b || !buf) return fail(QS_E_INVALID, "qs_branch_state: null argument");
  hipStream_t st = (hipStream_t)stream;
  b->h->fuse.forget();
  int which;
  switch (block) {
    case QS_STATE_AGENT: which = BR_AGENT; break;
    case QS_STATE_HISTORY: which = BR_HIST; break;
    case QS_STATE_ENV: {   // the external layout [4][C · E] int32, from the records
      HIP_TRY(hipSetDevice(b->h->device));
      const int V = (int)b->sz.V;
      env_io_kernel<<<(V + 255) / 256, 256, 0, st>>>((int32_t*)b->block(BR_ENV), buf, V, true, false, nullptr);
      HIP_TRY(hipGetLastError());
      return QS_OK;
    }
    default: return fail(QS_E_INVALID, "qs_branch_state: bad block (a branch set keeps no episode returns)");
  }
  HIP_TRY(hipSetDevice(b->h->device));
  HIP_TRY(hipMemcpyAsync(buf, b->block(which), b->sz.bytes[which], hipMemcpyDeviceToDevice, st));
  return QS_OK;
}

int qs_episode_log(qs_handle* h, qs_episode_rec* dst, int64_t cap, int64_t* total, int64_t* written, void* stream) {
  if (!h || !total) return fail(QS_E_INVALID, "qs_episode_log: null argument");
  if (written) *written = 0;
  hipStream_t st = (hipStream_t)stream;
  h->fuse.forget();
  HIP_TRY(hipSetDevice(h->device));
  const int E = h->dims.num_envs, R = h->log_per_env;
  const unsigned grid = (unsigned)((E + 255) / 256);
  if (!h->logw) HIP_TRY(hipMalloc((void**)&h->logw, sizeof(qs::LogWork)));
  qs::LogWork* w = h->logw;
  // 1. total and the newest seq (one 16-byte read back)
  HIP_TRY(hipMemsetAsync(w, 0, sizeof(qs::LogWork), st));
  HIP_TRY(hipMemsetAsync(&w->maxseq, 0xff, sizeof(long long), st));   // −1: nothing logged
  hipLaunchKernelGGL(qs::log_scan_kernel, dim3(grid), dim3(256), 0, st, h->env, h->log, E, R, w);
  HIP_TRY(hipGetLastError());
  struct { unsigned long long total; long long maxseq; } head;
  HIP_TRY(hipMemcpyAsync(&head, w, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total = (int64_t)head.total;
  if (!dst || cap <= 0 || head.total == 0) return QS_OK;
  // 2. how far below the newest seq the newest `cap` live records reach
  hipLaunchKernelGGL(qs::log_hist_kernel, dim3(grid), dim3(256), 0, st, h->env, h->log, E, R, w);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned int> hist(qs::kLogBins);
  HIP_TRY(hipMemcpyAsync(hist.data(), w->hist, hist.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t live = 0, cum = 0;
  for (unsigned int c : hist) live += c;
  long long thr = -1;   // every live record, unless the newest `cap` lie within the binned window
  uint64_t want = live;
  for (int b = 0; b < qs::kLogBins - 1; ++b) {
    cum += hist[b];
    if (cum >= (uint64_t)cap) {   // bin b = seq maxseq − b holds the cap-th newest
      thr = head.maxseq - b;
      want = cum;
      break;
    }
  }
  // 3. compact the records at or above the threshold (the cap newest plus the rest
  // of the threshold seq's ties) and order them on the host: (seq, env) is the
  // order the reference's env loop logs them
  if (h->log_sel_cap < want) {
    if (h->log_sel) HIP_TRY(hipFree(h->log_sel));
    h->log_sel = nullptr;
    h->log_sel_cap = std::max<size_t>((size_t)want, 1024);
    HIP_TRY(hipMalloc((void**)&h->log_sel, h->log_sel_cap * sizeof(qs_episode_rec)));
  }
  hipLaunchKernelGGL(qs::log_select_kernel, dim3(grid), dim3(256), 0, st, h->env, h->log, E, R, thr, h->log_sel,
                     (unsigned)want, w);
  HIP_TRY(hipGetLastError());
  std::vector<qs_episode_rec> sel((size_t)want);
  HIP_TRY(hipMemcpyAsync(sel.data(), h->log_sel, sel.size() * sizeof(qs_episode_rec), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const size_t k = std::min<size_t>(sel.size(), (size_t)cap);
  auto older = [](const qs_episode_rec& a, const qs_episode_rec& b) {
    return a.seq != b.seq ? a.seq < b.seq : a.env < b.env;
  };
  // the k newest, oldest first
  std::nth_element(sel.begin(), sel.begin() + (sel.size() - k), sel.end(), older);
  std::sort(sel.begin() + (sel.size() - k), sel.end(), older);
  HIP_TRY(hipMemcpyAsync(dst, sel.data() + (sel.size() - k), k * sizeof(qs_episode_rec), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (written) *written = (int64_t)k;
  return QS_OK;
}

int qs_reset_error(qs_handle* h, int* out) {
  if (!h || !out) return fail(QS_E_INVALID, "qs_reset_error: null argument");
  h->fuse.forget();
  HIP_TRY(hipMemcpy(out, h->err, sizeof(int), hipMemcpyDeviceToHost));
  return QS_OK;
}

int qs_calib_copy(float* dst, const float* src, int64_t n, void* stream) {
  if (!dst || !src || n < 0) return fail(QS_E_INVALID, "qs_calib_copy: bad argument");
  long long blocks = std::min<long long>((n + 255) / 256, 256LL * 8);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(qs::calib_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dst, src, (long long)n);
  HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // extern "C"
