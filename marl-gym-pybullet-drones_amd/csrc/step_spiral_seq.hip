// step_spiral_seq.hip — multi-step step-kernel instantiations that read caller-supplied
// actions (FUSE = 2) for QS_TASK_SPIRAL.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_SEQ(QS_TASK_SPIRAL)
