// Translation unit of the carried objects' weight in the rollout (osc_object_load.hpp): the compiled Dual-UR5 tree, float and double records.
#include "osc_object_load.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_object_loads(const ObjectLoadArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.grippers == 0u) return 0;
    hipLaunchKernelGGL((osc_object_load_kernel<TopoDualUr5, T>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_object_loads<float>(const ObjectLoadArgs&, hipStream_t);
template int launch_object_loads<double>(const ObjectLoadArgs&, hipStream_t);

}  // namespace irlosc
