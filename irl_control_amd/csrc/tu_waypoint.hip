// Translation unit of the waypoint cycler of the rollout (osc_waypoint.hpp), float and double records.
#include "osc_waypoint.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_waypoints(const WaypointArgs& a, hipStream_t st) {
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(osc_waypoint_kernel<T>, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}
template int launch_waypoints<float>(const WaypointArgs&, hipStream_t);
template int launch_waypoints<double>(const WaypointArgs&, hipStream_t);

}  // namespace irlosc
