// step_launch.h — launch entry of the step kernel for one task family.
#pragma once
#include "step_kernel.h"

namespace qs {
// Launches step_kernel<T, TASK, act, ...> (control frequency and physics chosen
// from cf/pf/ph).  Defined and explicitly instantiated in one translation unit
// per task family.  Returns false for an unknown action type.
// FUSE = 1: the multi-step instances (ParamsMany: P.nsteps steps per launch,
// P.io[]), in translation units of their own; FUSE = 2: those that read the
// steps' actions from ParamsSeq::act[], in further ones; FUSE = 3: the branch
// rollouts of qs_score (ParamsScore), in theirs; FUSE = 4: those of a branch set
// (qs_branch_advance, ParamsBranch), in theirs; FUSE = 5: the branch rollouts with a
// tracking cost (qs_track_score, ParamsTrack), in theirs; FUSE = 6: those with separation and
// obstacle terms too (qs_avoid_score, ParamsAvoid), in theirs.  `fn`, if given, receives the kernel's
// function pointer (what a graph kernel node names); `select_only` looks the
// kernel up without launching it.
template <class T, int TASK, int FUSE = 0>
bool launch_task(int act, int grid, size_t lds, hipStream_t st, const KernelParams<T, FUSE>& P, int cf, int pf, int ph,
                 const void** fn = nullptr, bool select_only = false);
// The shape-specialised multi-step instance (step_kernel HOT = 1; step_mh_hot.hip)
// for a launch qs::hot_shape_ok accepts: MultiHover, ONE_D_PID, 30 Hz, no extra
// forces, D = 8; `phys` picks DYN or PYB.
template <class T>
void launch_hot(int phys, int grid, size_t lds, hipStream_t st, const ParamsMany<T>& P, const void** fn = nullptr,
                bool select_only = false);
// The ring instance (step_kernel HOT = 2; step_mh_ring.hip) for a launch
// qs::ring_shape_ok accepts: the hot shape, P.nsteps steps over P.period output sets.
template <class T>
void launch_ring(int phys, int grid, size_t lds, hipStream_t st, const ParamsRing<T>& P, const void** fn = nullptr,
                 bool select_only = false);
}  // namespace qs
