// Translation unit of the wall kernel of the rollout (osc_wall.hpp): the compiled Dual-UR5 tree, float and double records.
#include "osc_wall.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_walls(const WallArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.devs == 0u) return 0;
    hipLaunchKernelGGL((osc_wall_kernel<TopoDualUr5, T>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_walls<float>(const WallArgs&, hipStream_t);
template int launch_walls<double>(const WallArgs&, hipStream_t);

}  // namespace irlosc
