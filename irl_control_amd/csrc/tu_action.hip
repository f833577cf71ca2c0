// Translation unit of the action list of the rollout (osc_action.hpp), float and double records, without and with a motion.
#include "osc_action.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_actions(const ActionArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(osc_action_kernel<T>, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_actions<float>(const ActionArgs&, hipStream_t);
template int launch_actions<double>(const ActionArgs&, hipStream_t);

template <typename T>
int launch_actions_motion(const ActionMotionArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL((osc_action_kernel<T, true>), dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_actions_motion<float>(const ActionMotionArgs&, hipStream_t);
template int launch_actions_motion<double>(const ActionMotionArgs&, hipStream_t);

}  // namespace irlosc
