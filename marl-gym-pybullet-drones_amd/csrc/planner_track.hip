// planner_track.hip — the tracking cost of the MPPI / CEM score stage (include/quadswarm.h,
// qs_track_fold, qs_track_mppi_set / qs_track_cem_set; DESIGN.md §4a "Tracking cost").
//
// The cost itself is summed inside the score launch (qs_track_score, the FUSE = 5 step
// kernel).  What lives here is the fold launch, which turns the launch's ret / ret_agent
// and cost_agent into the objective in place (float64, every operation rounded on its
// own, d ascending, one thread per (c, e), no atomics), and what a planner holds once a
// spec is attached: a tracking spec, an avoidance spec (qs_avoid_mppi_set /
// qs_avoid_cem_set: the FUSE = 6 step kernel behind qs_avoid_score) or both.  The host
// arithmetic (refusals, sizes, the fold's grid) is track_sizes.h and avoid_sizes.h.
#include "planner_common.h"
#include "track_sizes.h"
#include "avoid_sizes.h"

namespace {

// ret[v] = scale · ret[v] − (Σ_d cost[v][d]) / D;  ret_agent[v][d] = scale · ret_agent[v][d] − cost[v][d]
__global__ __launch_bounds__(qs::kTrackFoldThreads) void track_fold_kernel(int V, int D, double scale, double* ret,
                                                                            double* ret_agent, const double* cost) {
  const int v = (int)(blockIdx.x * (unsigned)qs::kTrackFoldThreads + threadIdx.x);
  if (v >= V) return;
  const size_t a0 = (size_t)v * (size_t)D;
  double sum = 0.0;
  for (int d = 0; d < D; ++d) {
    const double c = cost[a0 + d];
    sum = __dadd_rn(sum, c);
    if (ret_agent) ret_agent[a0 + d] = __dsub_rn(__dmul_rn(scale, ret_agent[a0 + d]), c);
  }
  if (ret) ret[v] = __dsub_rn(__dmul_rn(scale, ret[v]), __ddiv_rn(sum, (double)D));
}

int fold_launch(const char* who, int C, int E, int D, double scale, double* ret, double* ret_agent, const double* cost,
                hipStream_t st) {
  using qs::set_last_error;
  const std::string w = std::string(who) + ": ";
  if (!cost) return set_last_error(QS_E_INVALID, w + "cost_agent is null");
  if (!ret && !ret_agent) return set_last_error(QS_E_INVALID, w + "nothing to fold (ret and ret_agent are both null)");
  if (!std::isfinite(scale)) return set_last_error(QS_E_INVALID, w + "reward_scale must be finite");
  const uint32_t grid = qs::track_fold_grid(C, E);
  if (grid == 0 || D < 1 || (uint64_t)C * (uint64_t)E * (uint64_t)D >= (uint64_t(1) << 31))
    return set_last_error(QS_E_INVALID, w + "C, E and D must be >= 1 and C * E * D below 2^31");
  hipLaunchKernelGGL(track_fold_kernel, dim3(grid), dim3(qs::kTrackFoldThreads), 0, st, C * E, D, scale, ret, ret_agent,
                     cost);
  PLANNER_HIP_TRY(hipGetLastError());
  return QS_OK;
}

}  // namespace

namespace qs {

// What a planner holds once a tracking spec, an avoidance spec (qs_avoid_mppi_set /
// qs_avoid_cem_set; DESIGN.md §4a "Separation and obstacle terms") or both are attached:
// the two attach and detach independently and share the buffers.
struct TrackState {
  bool has_track, has_avoid;
  qs_track_spec spec;
  qs_avoid_spec avoid;
  double* cost_agent;   // [C][E][D]
  double* ret_agent;    // [C][E][D], an env-level planner's own (per-drone mode: null, the planner has one)
};

void track_release(PlannerBase* p) {
  if (!p->track) return;
  if (p->track->cost_agent) (void)hipFree(p->track->cost_agent);
  if (p->track->ret_agent) (void)hipFree(p->track->ret_agent);
  delete p->track;
  p->track = nullptr;
}

// A fresh state with zeroed buffers in place of the planner's (which may be null).
static int state_install(const std::string& w, PlannerBase* p, const TrackState& want) {
  TrackState* t = new (std::nothrow) TrackState(want);
  if (!t) return set_last_error(QS_E_NOMEM, w + "out of host memory");
  t->cost_agent = nullptr;
  t->ret_agent = nullptr;
  const uint64_t bytes = track_cost_bytes(p->C, p->E, p->D);   // (the planner's create has bounded C · E · D)
  hipError_t e = hipMalloc((void**)&t->cost_agent, bytes);
  if (e == hipSuccess) e = hipMemset(t->cost_agent, 0, bytes);
  if (e == hipSuccess && !p->per_drone) {
    e = hipMalloc((void**)&t->ret_agent, bytes);
    if (e == hipSuccess) e = hipMemset(t->ret_agent, 0, bytes);
  }
  if (e != hipSuccess) {
    if (t->cost_agent) (void)hipFree(t->cost_agent);
    if (t->ret_agent) (void)hipFree(t->ret_agent);
    delete t;
    return set_last_error(e == hipErrorOutOfMemory ? QS_E_NOMEM : QS_E_HIP, w + hipGetErrorString(e));
  }
  if (p->track) {   // replaced; the work in flight may still read the old buffers
    (void)hipDeviceSynchronize();
    track_release(p);
  }
  p->track = t;
  return QS_OK;
}

int track_attach(const char* who, PlannerBase* p, const qs_track_spec* spec) {
  const std::string w = std::string(who) + ": ";
  if (!p) return set_last_error(QS_E_INVALID, w + "null planner");
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (!spec) {   // detach; the work in flight may still read the buffers
    if (p->track && p->track->has_avoid) {   // the avoidance spec stays, and the buffers with it
      p->track->has_track = false;
      return QS_OK;
    }
    if (p->track) PLANNER_HIP_TRY(hipDeviceSynchronize());
    track_release(p);
    return QS_OK;
  }
  if (p->value)
    return set_last_error(QS_E_INVALID, w + "a value tail is attached: its discounted return and the undiscounted "
                                            "tracking cost do not compose (detach it first)");
  TrackSpecShape v;
  v.ref = (uintptr_t)spec->ref;
  v.L = spec->L;
  for (int k = 0; k < kTrackState; ++k) v.q[k] = spec->q[k];
  for (int k = 0; k < kTrackMaxAct; ++k) v.r[k] = spec->r[k];
  v.terminal = spec->terminal;
  v.reward_scale = spec->reward_scale;
  switch (track_refusal(v, p->E, p->D, p->A)) {
    case kTrackRefNull: return set_last_error(QS_E_INVALID, w + "ref is null");
    case kTrackRefAlign: return set_last_error(QS_E_INVALID, w + "ref must be 16-byte aligned");
    case kTrackRows: return set_last_error(QS_E_INVALID, w + "L must be >= 1");
    case kTrackQ: return set_last_error(QS_E_INVALID, w + "q[0 .. 11] must be finite and >= 0");
    case kTrackR: return set_last_error(QS_E_INVALID, w + "r[a] must be finite and >= 0 for each action component");
    case kTrackTerminal: return set_last_error(QS_E_INVALID, w + "terminal must be finite and >= 0");
    case kTrackScale: return set_last_error(QS_E_INVALID, w + "reward_scale must be finite");
    case kTrackOffsets:
      return set_last_error(QS_E_INVALID, w + "L * num_envs * num_drones * 48 bytes of ref are past the 32-bit offsets");
    default: break;
  }
  TrackState want{};
  if (p->track) want = *p->track;
  want.has_track = true;
  want.spec = *spec;
  return state_install(w, p, want);
}

int avoid_attach(const char* who, PlannerBase* p, const qs_avoid_spec* spec) {
  const std::string w = std::string(who) + ": ";
  if (!p) return set_last_error(QS_E_INVALID, w + "null planner");
  PLANNER_HIP_TRY(hipSetDevice(p->info.device));
  if (!spec) {   // detach; the work in flight may still read the buffers
    if (p->track && p->track->has_track) {   // the tracking spec stays, and the buffers with it
      p->track->has_avoid = false;
      return QS_OK;
    }
    if (p->track) PLANNER_HIP_TRY(hipDeviceSynchronize());
    track_release(p);
    return QS_OK;
  }
  if (p->value)
    return set_last_error(QS_E_INVALID, w + "a value tail is attached: its discounted return and the undiscounted "
                                            "avoidance cost do not compose (detach it first)");
  const AvoidSpecShape v{(uintptr_t)spec->obstacles, spec->M, spec->sep_radius, spec->sep_weight, spec->sep_z_scale};
  if (const char* why = avoid_refusal_text(avoid_refusal(v))) return set_last_error(QS_E_INVALID, w + why);
  TrackState want{};
  if (p->track) want = *p->track;
  want.has_avoid = true;
  want.avoid = *spec;
  return state_install(w, p, want);
}

bool track_attached(const PlannerBase* p) { return p->track != nullptr && p->track->has_track; }
bool avoid_attached(const PlannerBase* p) { return p->track != nullptr && p->track->has_avoid; }

int track_buffers(const char* who, const PlannerBase* p, double** cost_agent, double** ret_agent) {
  if (!p || !cost_agent || !ret_agent) return set_last_error(QS_E_INVALID, std::string(who) + ": null argument");
  const TrackState* t = p->track;
  *cost_agent = t ? t->cost_agent : nullptr;
  *ret_agent = t ? (p->per_drone ? (double*)p->ret_agent : t->ret_agent) : nullptr;
  return QS_OK;
}

// The score stage with a spec attached: qs_track_score (with an avoidance spec:
// qs_avoid_score, whose track is the tracking spec or null), then the fold of ret and
// ret_agent, so both hold the objective at their level.  The fold's scale is the tracking
// spec's reward_scale, or 1 without one.
int track_score(PlannerBase* p, void* ret, void* first_done, void* stream) {
  TrackState* t = p->track;
  const qs_score_out so{ret, (int32_t*)first_done};
  double* const ra = p->per_drone ? (double*)p->ret_agent : t->ret_agent;
  const qs_track_spec* const ts = t->has_track ? &t->spec : nullptr;
  if (t->has_avoid) {
    if (int rc = qs_avoid_score(p->h, p->n, p->C, p->steps.data(), nullptr, &so, ra, ts, &t->avoid, t->cost_agent, stream))
      return rc;
  } else if (int rc = qs_track_score(p->h, p->n, p->C, p->steps.data(), nullptr, &so, ra, ts, t->cost_agent, stream)) {
    return rc;
  }
  return fold_launch("qs_track_fold", p->C, p->E, p->D, ts ? (double)ts->reward_scale : 1.0, (double*)ret, ra,
                     t->cost_agent, (hipStream_t)stream);
}

}  // namespace qs

extern "C" {

int qs_track_fold(int C, int E, int D, double reward_scale, double* ret, double* ret_agent, const double* cost_agent,
                  void* stream) {
  return fold_launch("qs_track_fold", C, E, D, reward_scale, ret, ret_agent, cost_agent, (hipStream_t)stream);
}

}  // extern "C"
