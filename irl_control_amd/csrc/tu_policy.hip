// Translation unit of the policy of the rollout (osc_policy.hpp), float and double records.
#include "osc_policy.hpp"
#include "launchers.hpp"

namespace irlosc {

template <typename T>
int launch_policy(const PolicyArgs& a, hipStream_t st) {
    if (a.t.B <= 0) return 0;
    const size_t lds = policy_lds_bytes<T>(a.net, a.t.ndev);
    if (lds > (size_t)64 << 10) {                   // beyond the default limit of a block's dynamic LDS: the largest networks
        const hipError_t e = hipFuncSetAttribute((const void*)osc_policy_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(osc_policy_kernel<T>, dim3((a.t.B + 63) / 64), dim3(64 * POLICY_WAVES), lds, st, a);
    return (int)hipGetLastError();
}
template int launch_policy<float>(const PolicyArgs&, hipStream_t);
template int launch_policy<double>(const PolicyArgs&, hipStream_t);

}  // namespace irlosc
