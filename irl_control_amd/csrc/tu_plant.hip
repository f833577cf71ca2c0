// Translation unit of the plant kernel of the rollout (osc_plant.hpp): the compiled Dual-UR5 tree, float and double records.
#include "osc_plant.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_plant(const PlantArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL((osc_plant_lane_kernel<TopoDualUr5, T>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_plant<float>(const PlantArgs&, hipStream_t);
template int launch_plant<double>(const PlantArgs&, hipStream_t);

int plant_joints() { return TopoDualUr5::NJ; }

}  // namespace irlosc
