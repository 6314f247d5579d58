// step_launch_impl.h — kernel launch dispatch, included by the per-task-family
// translation units (step_mh.hip, step_spiral.hip, step_marl.hip and their
// *_fused.hip twins, step_mh_seq.hip, step_spiral_seq.hip, step_mh_score.hip,
// step_spiral_score.hip, step_mh_branch.hip, step_spiral_branch.hip, step_mh_track.hip,
// step_spiral_track.hip, step_mh_avoid.hip and step_spiral_avoid.hip) so the
// kernel instantiations compile in parallel.
#pragma once
#include "step_launch.h"

namespace qs {

template <class T, int TASK, int ACT, int FUSE>
static void launch_one(int grid, size_t lds, hipStream_t st, const KernelParams<T, FUSE>& P, int ctrl_freq, int pyb_freq,
                       int phys, const void** fn, bool select_only) {
  constexpr int kCF = TASK == QS_TASK_SPIRAL ? 48 : 30;   // SpiralAviary.py:28; MH:20 and the MARL tasks
  const bool cf = ctrl_freq == kCF && pyb_freq == 240;
  // the default control frequency is compile-time (constant substeps/history);
  // no extra forces / downwash only / general force set (step_kernel AUXM)
  const int auxm = P.aux == 0 ? 0 : (P.aux == QS_AUX_DW ? 1 : 2);
  auto go = [&](auto kern) {
    if (fn) *fn = reinterpret_cast<const void*>(kern);
    if (!select_only) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, P);
  };
  if (P.flags & QS_FLAG_CF2P) {   // DroneModel.CF2P: the general substep (AUXM 3), run-time frequency
    if (phys == QS_PHYS_DYN) go(step_kernel<T, TASK, ACT, 0, QS_PHYS_DYN, 3, FUSE>);
    else go(step_kernel<T, TASK, ACT, 0, QS_PHYS_PYB, 3, FUSE>);
    return;
  }
  if (phys == QS_PHYS_DYN) {
    if (!cf) go(step_kernel<T, TASK, ACT, 0, QS_PHYS_DYN, 2, FUSE>);
    else if (auxm == 0) go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_DYN, 0, FUSE>);
    else if (auxm == 1) go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_DYN, 1, FUSE>);
    else go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_DYN, 2, FUSE>);
  } else {
    if (!cf) go(step_kernel<T, TASK, ACT, 0, QS_PHYS_PYB, 2, FUSE>);
    else if (auxm == 0) go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_PYB, 0, FUSE>);
    else if (auxm == 1) go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_PYB, 1, FUSE>);
    else go(step_kernel<T, TASK, ACT, kCF, QS_PHYS_PYB, 2, FUSE>);
  }
}

template <class T, int TASK, int FUSE>
bool launch_task(int act, int grid, size_t lds, hipStream_t st, const KernelParams<T, FUSE>& P, int cf, int pf, int ph,
                 const void** fn, bool select_only) {
  switch (act) {
    case QS_ACT_RPM: launch_one<T, TASK, QS_ACT_RPM, FUSE>(grid, lds, st, P, cf, pf, ph, fn, select_only); break;
    case QS_ACT_PID: launch_one<T, TASK, QS_ACT_PID, FUSE>(grid, lds, st, P, cf, pf, ph, fn, select_only); break;
    case QS_ACT_VEL: launch_one<T, TASK, QS_ACT_VEL, FUSE>(grid, lds, st, P, cf, pf, ph, fn, select_only); break;
    case QS_ACT_ONE_D_RPM: launch_one<T, TASK, QS_ACT_ONE_D_RPM, FUSE>(grid, lds, st, P, cf, pf, ph, fn, select_only); break;
    case QS_ACT_ONE_D_PID: launch_one<T, TASK, QS_ACT_ONE_D_PID, FUSE>(grid, lds, st, P, cf, pf, ph, fn, select_only); break;
    default: return false;
  }
  return true;
}


}  // namespace qs

#define QS_INSTANTIATE_LAUNCH_AS(TASK, FUSE)                                                                     \
  template bool qs::launch_task<float, TASK, FUSE>(int, int, size_t, hipStream_t,                               \
                                                   const qs::KernelParams<float, FUSE>&, int, int, int,         \
                                                   const void**, bool);                                         \
  template bool qs::launch_task<double, TASK, FUSE>(int, int, size_t, hipStream_t,                              \
                                                    const qs::KernelParams<double, FUSE>&, int, int, int,       \
                                                    const void**, bool);
#define QS_INSTANTIATE_LAUNCH(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 0)
#define QS_INSTANTIATE_LAUNCH_FUSED(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 1)
#define QS_INSTANTIATE_LAUNCH_SEQ(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 2)
#define QS_INSTANTIATE_LAUNCH_SCORE(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 3)
#define QS_INSTANTIATE_LAUNCH_BRANCH(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 4)
#define QS_INSTANTIATE_LAUNCH_TRACK(TASK) QS_INSTANTIATE_LAUNCH_AS(TASK, 5)
