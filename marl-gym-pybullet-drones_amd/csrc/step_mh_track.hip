// step_mh_track.hip — branch-rollout step-kernel instantiations with a tracking cost
// (FUSE = 5, qs_track_score: the FUSE = 3 launch that also sums each drone's quadratic
// cost against a caller-supplied reference) for QS_TASK_MULTIHOVER.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_TRACK(QS_TASK_MULTIHOVER)
