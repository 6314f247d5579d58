// step_spiral_score.hip — branch-rollout step-kernel instantiations (FUSE = 3, qs_score:
// candidate action sequences from the handle's state, nothing stored to it) for
// QS_TASK_SPIRAL.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_SCORE(QS_TASK_SPIRAL)
