// step_mh_avoid.hip — branch-rollout step-kernel instantiations with separation and
// obstacle terms (FUSE = 6, qs_avoid_score: the FUSE = 5 launch whose cost also holds a
// pairwise hinge among an env's drones and one against a caller-supplied obstacle
// table) for QS_TASK_MULTIHOVER.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_AS(QS_TASK_MULTIHOVER, 6)
