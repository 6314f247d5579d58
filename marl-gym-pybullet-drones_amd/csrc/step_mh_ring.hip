// step_mh_ring.hip — the ring instances (step_kernel HOT = 2) of QS_TASK_MULTIHOVER: the
// shape-specialised multi-step body of step_mh_hot.hip for the launches qs::ring_shape_ok
// (step_fuse.h) accepts, whose steps cycle through ParamsRing::period output sets.  DYN and
// PYB, fp32 and fp64: four kernels.
#include "step_launch.h"

namespace qs {

template <class T>
void launch_ring(int phys, int grid, size_t lds, hipStream_t st, const ParamsRing<T>& P, const void** fn, bool select_only) {
  auto go = [&](auto kern) {
    if (fn) *fn = reinterpret_cast<const void*>(kern);
    if (!select_only) hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, P);
  };
  if (phys == QS_PHYS_DYN) go(step_kernel<T, QS_TASK_MULTIHOVER, QS_ACT_ONE_D_PID, 30, QS_PHYS_DYN, 0, 1, 2>);
  else go(step_kernel<T, QS_TASK_MULTIHOVER, QS_ACT_ONE_D_PID, 30, QS_PHYS_PYB, 0, 1, 2>);
}

template void launch_ring<float>(int, int, size_t, hipStream_t, const ParamsRing<float>&, const void**, bool);
template void launch_ring<double>(int, int, size_t, hipStream_t, const ParamsRing<double>&, const void**, bool);

}  // namespace qs
