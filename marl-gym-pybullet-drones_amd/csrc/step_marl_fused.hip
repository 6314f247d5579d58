// step_marl_fused.hip — multi-step (FUSE) step-kernel instantiations for the
// Flock / Meetup / LeaderFollower family.
#include "step_launch_impl.h"

QS_INSTANTIATE_LAUNCH_FUSED(qs::kTaskMarl)
