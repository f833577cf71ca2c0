// Translation unit of the push kernel of the rollout (osc_push.hpp): the compiled Dual-UR5 tree, float and double records.
#include "osc_push.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_pushes(const PushArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.active == 0u) return 0;
    hipLaunchKernelGGL((osc_push_kernel<TopoDualUr5, T>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_pushes<float>(const PushArgs&, hipStream_t);
template int launch_pushes<double>(const PushArgs&, hipStream_t);

}  // namespace irlosc
