// Translation unit of the action-object kernel of the rollout (osc_object.hpp); float64 whatever the record type.
#include "osc_object.hpp"
#include "launchers.hpp"

namespace irlosc {

int launch_objects(const ObjectArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.nobj <= 0) return 0;
    hipLaunchKernelGGL(osc_object_kernel<IRLOSC_MAX_GRIPPERS>, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace irlosc
