// Translation unit of the joint-row kernel of the rollout (osc_joint.hpp): the compiled Dual-UR5 tree; float64 whatever the record type.
#include "osc_joint.hpp"
#include "topo_dual_ur5.hpp"
#include "launchers.hpp"

namespace irlosc {

int launch_joints(const JointArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.R <= 0) return 0;
    hipLaunchKernelGGL((osc_joint_kernel<TopoDualUr5>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace irlosc
