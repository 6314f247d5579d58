// step_mh_hot.hip — the shape-specialised multi-step instances (step_kernel HOT = 1) of
// QS_TASK_MULTIHOVER: ONE_D_PID at 30 Hz without extra forces, D = 8, for the launches
// qs::hot_shape_ok (step_fuse.h) accepts.  DYN and PYB, fp32 and fp64: four kernels.
#include "step_launch.h"

namespace qs {

template <class T>
void launch_hot(int phys, int grid, size_t lds, hipStream_t st, const ParamsMany<T>& P, const void** fn, bool select_only) {
  auto go = [&](auto kern) {
    if (fn) *fn = reinterpret_cast<const void*>(kern);
    if (!select_only) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, P);
  };
  if (phys == QS_PHYS_DYN) go(step_kernel<T, QS_TASK_MULTIHOVER, QS_ACT_ONE_D_PID, 30, QS_PHYS_DYN, 0, 1, 1>);
  else go(step_kernel<T, QS_TASK_MULTIHOVER, QS_ACT_ONE_D_PID, 30, QS_PHYS_PYB, 0, 1, 1>);
}

template void launch_hot<float>(int, int, size_t, hipStream_t, const ParamsMany<float>&, const void**, bool);
template void launch_hot<double>(int, int, size_t, hipStream_t, const ParamsMany<double>&, const void**, bool);

}  // namespace qs
