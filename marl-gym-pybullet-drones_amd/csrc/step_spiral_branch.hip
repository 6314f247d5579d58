// step_spiral_branch.hip — branch-set step-kernel instantiations (FUSE = 4,
// qs_branch_advance: the branch rollout whose virtual envs keep their state in a
// branch set from launch to launch) for QS_TASK_SPIRAL.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_BRANCH(QS_TASK_SPIRAL)
