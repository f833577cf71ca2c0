// Translation unit of the policy of the rollout (osc_policy.hpp), float and double records.
#include "osc_policy.hpp"
#include "launchers.hpp"

namespace irlosc {

// (a slot without a Gaussian head -- a.st.act == nullptr -- launches the NOISE = false form: the kernel it launched before there was a head)
template <typename T, bool NOISE>
static int launch_policy_form(const PolicyArgs& a, hipStream_t st) {
    const size_t lds = policy_lds_bytes<T>(a.net, a.t.ndev, NOISE);
    if (lds > (size_t)64 << 10) {                   // beyond the default limit of a block's dynamic LDS: the largest networks
        const hipError_t e = hipFuncSetAttribute((const void*)osc_policy_kernel<T, NOISE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((osc_policy_kernel<T, NOISE>), dim3((a.t.B + 63) / 64), dim3(64 * POLICY_WAVES), lds, st, a);
    return (int)hipGetLastError();
}
template <typename T>
int launch_policy(const PolicyArgs& a, hipStream_t st) {
    if (a.t.B <= 0) return 0;
    return a.st.act ? launch_policy_form<T, true>(a, st) : launch_policy_form<T, false>(a, st);
}
template int launch_policy<float>(const PolicyArgs&, hipStream_t);
template int launch_policy<double>(const PolicyArgs&, hipStream_t);

}  // namespace irlosc
