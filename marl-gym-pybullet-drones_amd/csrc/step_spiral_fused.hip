// step_spiral_fused.hip — multi-step (FUSE) step-kernel instantiations for QS_TASK_SPIRAL.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_FUSED(QS_TASK_SPIRAL)
