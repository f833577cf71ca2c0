// Translation unit of the teleoperation stream of the rollout (osc_teleop.hpp), float and double records.
#include "osc_teleop.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_teleop(const TeleopArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(osc_teleop_kernel<T>, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_teleop<float>(const TeleopArgs&, hipStream_t);
template int launch_teleop<double>(const TeleopArgs&, hipStream_t);

}  // namespace irlosc
